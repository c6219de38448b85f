// MCTS over SCS game trees on the device, lock-step, with the leaf evaluations supplied from
// outside (C ABI nz_scs_search_* / nz_scs_select / nz_scs_expand ...).  One wavefront owns one
// game: lane j scores child j of the node being left (up to 64 children), lane 0 runs the rules
// (scs_dev.hpp) on the game's scratch state.
//
// Reference semantics (paths relative to the reference repo), as tree_dev.hpp, with the numeric
// types SCS produces under numpy >= 2 (SURVEY.md section 8a row 3, appendix A rule 11):
//   * expansion priors are float32: softmax probs (float32) * int8 mask, np.sum in float32
//     (pairwise), float32 division                                  (Search/Explorer.py:165-179)
//   * score() with a float32 prior runs in float32: the Python floats u, c and q are cast to
//     float32 before each operation                                  (Search/Explorer.py:114-130)
//   * root noise makes the root's children's priors float64 (float32 * (1 - frac) rounded to
//     float32, plus the float64 noise term); from then on their score is float64
//                                                                    (Search/Explorer.py:201-210)
//   * SCS players are 0 and 1, so `parent.to_play == 2` never negates Q (appendix A rule 6)
// The tree arithmetic must not be contracted: this file is compiled with -ffp-contract=off.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/nuzero_amd.h"
#include "scs_dev.hpp"
#include "scs_agents.hpp"
#include "scs_openings.hpp"
#include "boardnet_internal.h"
#include "hip_own.hpp"

using namespace nz;

namespace {

// Children per node and decisions per game are bounded from the game description when the engine is created
// (nz_scs_search_create: `scs_limits`), not by constants: a wavefront handles a node's children in chunks of 64 lanes.
constexpr int MAXC_CHUNKS = 4;                 // chunks of 64 children a node may have
constexpr int MAXC_LIMIT = 64 * MAXC_CHUNKS;   // 256: more legal actions than that in one position are rejected at create
constexpr int MAX_ACTIONS = 21 * SCS_MAX_TILES;
constexpr int MASK_WORDS = (MAX_ACTIONS + 31) / 32;

struct SNode {                    // array-of-structures: one 32-byte record per node
  double prior;                   // float32 value unless prior_f64
  double value_sum;
  int32_t visit;
  int32_t child_base;
  uint16_t n_children;
  uint16_t action;
  int8_t to_play;                 // -1 until evaluated
  int8_t prior_f64;               // 1: prior went through the root-noise mix (float64 arithmetic)
  int8_t terminal;
  int8_t pad;
};

struct SearchParams {
  int32_t n_games, cap, sims, training, softmax_moves, negate_player, tab_len, max_path;
  double frac, one_minus_frac, value_factor, eps_softmax, eps_random;
  const double* bias_tab;
  const double* sqrt_tab;
  const ScsRules* rules;   // the game description; with per-game maps (nz_scs_search_set_games) one row per game of the round
  const int32_t* rules_row;  // [G] the row of `rules` each slot's game reads, or nullptr: all read row 0
  const uint64_t* rules_key; // [rows][2] digest of each row's map, mixed into the cache key (nullptr: one map, not mixed in)
  ScsState* real;          // [G]
  ScsState* scratch;       // [G]
  SNode* nodes;            // [G][2][half_cap]: two halves per game, the live tree is in half `half[g]`
  int8_t* half;            // [G]
  int32_t half_cap;
  int32_t* node_count;     // [G]
  int32_t* root;           // [G]
  int32_t* sims_left;      // [G]
  int32_t* pending;        // [G] leaf slot or -1
  int32_t* path;           // [G][max_path]
  int32_t* path_len;       // [G]
  uint32_t* leaf_mask;     // [G][MASK_WORDS] legal actions at the pending leaf
  int32_t* leaf_count;     // [1]
  int32_t* active_count;   // [1] games that are not done with their move after a wave
  int32_t* clear_counters; // the (leaf, active) pair of the NEXT wave, zeroed by this one (nullptr: the host zeroes)
  // numpy's pairwise float32 sum over num_actions entries as a straight program: leaf blocks [pw_hi[b-1], pw_hi[b])
  // in index order, eight strided partial sums up to pw_be[b] and the rest added one by one, then pw_merge[b]
  // "left + right" merges of the block-sum stack (built on the host for this game's num_actions)
  int32_t num_actions;
  int32_t pw_blocks;
  uint16_t pw_hi[48], pw_be[48];
  uint8_t pw_merge[48];
  int32_t maxc;            // children per node the records hold (a multiple of 64, <= MAXC_LIMIT)
  int32_t max_moves;       // decisions per game the records hold
  int32_t terminal_budget; // simulations ending in terminal leaves one game may run per wave
  int32_t image_row_stride; // > 0: leaf images are written as input rows of a board net (floats per row), else NCHW
  // inference cache (keyless hash table shared by the games of the engine, see cache_put_kernel); c_bits == 0: off
  int32_t c_bits;          // log2(entries)
  int32_t c_wave;          // serial number of this simulation wave (arbitration of same-wave writers)
  int32_t c_hit_base;      // evaluation slots [c_hit_base, c_hit_base + G) receive this wave's cache hits
  uint64_t* c_id;          // [entries][2] the 128-bit hash of the state an entry holds (0, 0: empty)
  float* c_probs;          // [entries][A] post-softmax probabilities
  float* c_value;          // [entries]
  int32_t* c_writer;       // [entries] last wave that wrote the entry (wave-by-wave route)
  uint64_t* c_check;       // [entries] check word over (key, probabilities, value) (persistent route: self-validating entries)
  uint64_t* leaf_key;      // [G][2] hash of each queued (missed) leaf, by evaluation slot
  int32_t* hit_count;      // [1] hits of this wave
  float* eval_probs;       // [3 G][A] evaluations: the network's [0, G), cache hits [G, 2 G) / [2 G, 3 G) by wave parity
  float* eval_value;       // [3 G]
  int32_t* error_flag;     // [3] the flag word (FLAG_TEXT); game and decision of the first root found without a legal action (-1, -1: none)
  int64_t* counters;       // [16] simulations, expansions; [8] cache hits, [9] misses, [10] entries in use; [2..7] shader ticks per phase of the NZ_SCS_STAMPS diagnostic build
  // records [G][max_moves]...
  int32_t* rec_action;
  int32_t* rec_tree_size;
  int32_t* rec_children;
  double* rec_bias;
  double* rec_root_value_sum;
  int32_t* rec_child_action;   // [G][max_moves][maxc]
  int32_t* rec_child_visit;
  double* rec_child_prior;
  double* rec_child_value_sum;
};

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
template <typename T>
__device__ __forceinline__ T wave_get(T v, int lane) { return __shfl(v, lane, 64); }

// Wavefront-wide max over (score, key) tuples, the larger key winning a tie (Explorer.py:100: max over (score, action,
// child) tuples; key = action << 8 | child index).  Inside each 16-lane row two butterflies of DPP rotations (the maximum
// score, then the largest key among the lanes that hold it), then the four rows' results meet through v_readlane: no
// trip through the LDS crossbar (six rounds of three ds_bpermute were a thousand cycles per tree level).  Lanes without
// a child pass score = -inf, key = -1.  Returns the winning key in every lane.
template <int N>
__device__ __forceinline__ int dpp_row_ror(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x120 + N, 0xF, 0xF, false); }
template <int N>
__device__ __forceinline__ double dpp_row_ror(double v) {
  return __hiloint2double(dpp_row_ror<N>(__double2hiint(v)), dpp_row_ror<N>(__double2loint(v)));
}
__device__ __forceinline__ int wave_argmax_key(double score, int key) {
  double m = score;
  m = fmax(m, dpp_row_ror<8>(m));
  m = fmax(m, dpp_row_ror<4>(m));
  m = fmax(m, dpp_row_ror<2>(m));
  m = fmax(m, dpp_row_ror<1>(m));
  int win = (score == m) ? key : -1;
  win = max(win, dpp_row_ror<8>(win));
  win = max(win, dpp_row_ror<4>(win));
  win = max(win, dpp_row_ror<2>(win));
  win = max(win, dpp_row_ror<1>(win));
  double best = -INFINITY;
  int best_key = -1;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double mr = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(m), 16 * r),
                                       __builtin_amdgcn_readlane(__double2loint(m), 16 * r));
    const int kr = __builtin_amdgcn_readlane(win, 16 * r);
    if (mr > best || (mr == best && kr > best_key)) { best = mr; best_key = kr; }
  }
  return best_key;
}

// score of one child (Explorer.score, :114-130) in the reference's dtypes
__device__ __forceinline__ double child_score(const SearchParams& p, const SNode& c, double sq, double cb, bool negate) {
  const double u = sq / (double)(c.visit + 1);
  double q = (c.visit == 0) ? 0.0 : c.value_sum / (double)c.visit;
  if (negate) q = -q;
  q = q * p.value_factor;
  if (c.prior_f64) {
    double conf = c.prior * u;
    conf = conf * cb;
    return conf + q;
  }
  float conf = (float)c.prior * (float)u;
  conf = conf * (float)cb;
  return (double)(conf + (float)q);
}

// numpy's float32 pairwise sum (np.sum over all num_actions entries of `probs`, Explorer.py:169) of an array that
// is zero except at k sorted positions; adding a zero is exact, so only the non-zero entries and numpy's block
// structure matter.  Wave-uniform: lane i holds the i-th non-zero entry (idx ascending, val), every lane walks the
// block program of SearchParams (built on the host) with the entries broadcast by v_readlane -- no memory accesses.
// Entry j lives in lane j & 63 of register j >> 6 (up to MAXC_CHUNKS registers per lane).
template <int CH = MAXC_CHUNKS>
__device__ __forceinline__ float np_sum_sparse_f32_wave(const SearchParams& p, const int (&idx)[CH],
                                                        const float (&val)[CH], int k) {
  float st0 = 0.f, st1 = 0.f, st2 = 0.f, st3 = 0.f, st4 = 0.f, st5 = 0.f, st6 = 0.f, st7 = 0.f;   // block-sum stack
  int sp = 0, i = 0, lo = 0;
  auto entry_idx = [&](int j) {
    const int c = __builtin_amdgcn_readfirstlane(j >> 6), l = __builtin_amdgcn_readfirstlane(j & 63);
    int r = idx[0];
    if constexpr (CH > 1) r = c == 0 ? idx[0] : c == 1 ? idx[1] : c == 2 ? idx[2 % CH] : idx[3 % CH];
    return __builtin_amdgcn_readlane(r, l);
  };
  auto entry_val = [&](int j) {
    const int c = __builtin_amdgcn_readfirstlane(j >> 6), l = __builtin_amdgcn_readfirstlane(j & 63);
    float r = val[0];
    if constexpr (CH > 1) r = c == 0 ? val[0] : c == 1 ? val[1] : c == 2 ? val[2 % CH] : val[3 % CH];
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r), l));
  };
  for (int b = 0; b < p.pw_blocks; ++b) {
    const int hi = p.pw_hi[b], be = p.pw_be[b];
    // numpy's eight running sums r[0..7] of the block live in lanes 0..7 (one compare and one add per entry instead of
    // eight of each); adding 0.0f to the other seven is exact
    float racc = 0.f;
    const int lane8 = (int)(threadIdx.x & 63);
    while (i < k) {
      const int ix = entry_idx(i);
      if (ix >= be) break;
      const float v = entry_val(i);
      racc += lane8 == ((ix - lo) & 7) ? v : 0.f;
      ++i;
    }
    // ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), read from lane 0: lane i takes lane i + 1 / + 2 / + 4 of its
    // row by DPP shifts (only lane 0's chain matters; no trip through the LDS crossbar)
    const float t1 = racc + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, racc), 0x101, 0xF, 0xF, false));   // row_shl:1
    const float t2 = t1 + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, t1), 0x102, 0xF, 0xF, false));       // row_shl:2
    const float t3 = t2 + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, t2), 0x104, 0xF, 0xF, false));       // row_shl:4
    float res = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, t3)));
    while (i < k) {
      if (entry_idx(i) >= hi) break;
      res = res + entry_val(i);
      ++i;
    }
    for (int mrg = p.pw_merge[b];; --mrg) {            // push, then merge: left + right
      switch (sp) {
        case 0: st0 = res; break; case 1: st1 = res; break; case 2: st2 = res; break; case 3: st3 = res; break;
        case 4: st4 = res; break; case 5: st5 = res; break; case 6: st6 = res; break; default: st7 = res; break;
      }
      ++sp;
      if (mrg == 0) break;
      float right, left;
      switch (sp) {
        case 2: left = st0; right = st1; break; case 3: left = st1; right = st2; break; case 4: left = st2; right = st3; break;
        case 5: left = st3; right = st4; break; case 6: left = st4; right = st5; break; case 7: left = st5; right = st6; break;
        default: left = st6; right = st7; break;
      }
      res = left + right;
      sp -= 2;
    }
    lo = hi;
  }
  return st0;
}
// numpy's pairwise sum of a dense float64 vector (the children of one node: n <= MAXC_LIMIT = 256): blocks of at most 128
// entries on eight running sums; a longer vector is halved (the left half a multiple of eight) and the halves' sums are
// added -- two levels of halving reach every n <= 256 (no recursion on the device: DEPTH counts them down)
__device__ inline double np_sum_f64_block(const double* v, int n) {     // n <= 128
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r = r + v[i];
    return r;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = v[j];
  int i = 8;
  for (; i < n - n % 8; i += 8)
    for (int j = 0; j < 8; ++j) r[j] = r[j] + v[i + j];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res = res + v[i];
  return res;
}
template <int DEPTH = 2>
__device__ inline double np_sum_f64(const double* v, int n) {
  if constexpr (DEPTH > 0) {
    if (n > 128) {
      int n2 = n / 2;
      n2 -= n2 % 8;
      const double left = np_sum_f64<DEPTH - 1>(v, n2);
      return left + np_sum_f64<DEPTH - 1>(v + n2, n - n2);
    }
  }
  return np_sum_f64_block(v, n);
}
static_assert(MAXC_LIMIT <= 256, "np_sum_f64 halves a vector at most twice");

__device__ __forceinline__ const ScsRules& rules_of(const SearchParams& p, int g) {
  return p.rules[p.rules_row ? p.rules_row[g] : 0];
}

// the half of game g's arena that holds its live tree
__device__ __forceinline__ SNode* arena(const SearchParams& p, int g) {
  return p.nodes + (size_t)g * p.cap + (size_t)p.half[g] * p.half_cap;
}

// a node nobody has visited or evaluated: the root of a new game (prior 0, action 0), a fresh child of an expansion
__device__ __forceinline__ SNode blank_node(double prior, int action) {
  SNode n;
  n.prior = prior; n.value_sum = 0.0; n.visit = 0; n.child_base = 0; n.n_children = 0; n.action = (uint16_t)action;
  n.to_play = -1; n.prior_f64 = 0; n.terminal = 0; n.pad = 0;
  return n;
}

// slot g starts a new game: the rules' initial state, a tree of one blank root in half 0 of the arena, no records
__device__ __forceinline__ void reset_slot(const SearchParams& p, int g) {
  Scs(rules_of(p, g), p.real[g]).reset();
  p.half[g] = 0;
  p.nodes[(size_t)g * p.cap] = blank_node(0.0, 0);
  p.node_count[g] = 1;
  p.root[g] = 0;
  p.sims_left[g] = 0;
  p.pending[g] = -1;
  p.path_len[g] = 0;
  for (int m = 0; m < p.max_moves; ++m) {
    p.rec_action[(size_t)g * p.max_moves + m] = -1;
    p.rec_children[(size_t)g * p.max_moves + m] = 0;
    p.rec_tree_size[(size_t)g * p.max_moves + m] = 0;
  }
}

__global__ void search_reset_kernel(SearchParams p) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) {
    *p.leaf_count = 0; *p.active_count = 0; *p.error_flag = 0;
    p.error_flag[1] = -1; p.error_flag[2] = -1;
    for (int i = 0; i < 16; ++i)
      if (i < 8 || i > 10) p.counters[i] = 0;      // [8..10] belong to the inference cache (nz_scs_search_cache)
  }
  if (g < p.n_games) reset_slot(p, g);
}

// ---- rounds of more games than slots (nz_scs_search_play_round) ----------------------------------------------------
// A finished game's records leave its slot for the round's store (one row per game of the round), then the slot starts
// the next game of the round: Gamer actors play their games back to back (Gamer.py:45-98), and a round ends no later
// than its longest game instead of idling every slot whose game was short.
struct RoundStore {
  int32_t *action, *tree_size, *children, *child_action, *child_visit, *status;   // status [n][2]: length, terminal value
  double *bias, *root_value_sum, *child_prior, *child_value_sum;
};
// one workgroup per slot; `to_record[g]` = row of the store that takes slot g's game, or -1
__global__ void archive_kernel(SearchParams p, RoundStore st, const int32_t* __restrict__ to_record) {
  const int g = blockIdx.x;
  const int rec = to_record[g];
  if (rec < 0) return;
  const ScsState& real = p.real[g];
  const int M = p.max_moves, MAXC = p.maxc;
  const int len = real.length < M ? real.length : M;
  const size_t src = (size_t)g * M, dst = (size_t)rec * M;
  for (int m = threadIdx.x; m < M; m += blockDim.x) {
    const bool played = m < len;
    st.action[dst + m] = played ? p.rec_action[src + m] : -1;
    st.tree_size[dst + m] = played ? p.rec_tree_size[src + m] : 0;
    st.children[dst + m] = played ? p.rec_children[src + m] : 0;
    st.bias[dst + m] = played ? p.rec_bias[src + m] : 0.0;
    st.root_value_sum[dst + m] = played ? p.rec_root_value_sum[src + m] : 0.0;
  }
  for (int i = threadIdx.x; i < len * MAXC; i += blockDim.x) {
    const int m = i / MAXC, j = i - m * MAXC;
    if (j < p.rec_children[src + m]) {
      st.child_action[dst * MAXC + i] = p.rec_child_action[src * MAXC + i];
      st.child_visit[dst * MAXC + i] = p.rec_child_visit[src * MAXC + i];
      st.child_prior[dst * MAXC + i] = p.rec_child_prior[src * MAXC + i];
      st.child_value_sum[dst * MAXC + i] = p.rec_child_value_sum[src * MAXC + i];
    }
  }
  if (threadIdx.x == 0) {
    st.status[rec * 2] = real.length;
    st.status[rec * 2 + 1] = real.terminal_value;
  }
}
// search_reset_kernel for the slots with restart[g] != 0 (counters and flags are the round's: untouched)
__global__ void restart_kernel(SearchParams p, const int32_t* __restrict__ restart) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < p.n_games && restart[g]) reset_slot(p, g);
}

// children of each live game's root (the number of gamma draws of the next move)
__global__ void root_children_kernel(SearchParams p, int32_t* out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.n_games) return;
  out[g] = p.real[g].terminal ? 0 : arena(p, g)[p.root[g]].n_children;
}

// add_exploration_noise (Explorer.py:201-210) and the start of a move's search
__global__ void begin_move_kernel(SearchParams p, const double* __restrict__ noise) {
  const int g = blockIdx.x;
  const int lane = lane_id();
  if (p.real[g].terminal) return;
  SNode* nodes = arena(p, g);
  const SNode& root = nodes[p.root[g]];
  for (int j = lane; p.training && j < root.n_children; j += 64) {
    SNode& c = nodes[root.child_base + j];
    const double n = noise[(size_t)g * p.maxc + j];
    double a;
    if (c.prior_f64) a = c.prior * p.one_minus_frac;
    else a = (double)((float)c.prior * (float)p.one_minus_frac);
    const double b = n * p.frac;
    c.prior = a + b;
    c.prior_f64 = 1;
  }
  if (lane == 0) {
    p.sims_left[g] = p.sims;
    p.pending[g] = -1;
  }
}

// ---- inference cache ------------------------------------------------------------------------------------------
// The reference's optional cache (Explorer.py:146-155; Utils/Caches/KeylessCache.py:24-160: hash of the state tensor,
// index bits select the slot, the remaining bits are stored as the entry's id; no keys kept) as one device table
// shared by all games of the engine.  Key: a 128-bit hash of what the tensor is generated from -- the game STATE and,
// with per-game maps, the digest of the game's map (terrain and victory points are image planes that ScsState does not
// hold; equal states on equal maps give equal tensors, so a hit returns what the network would compute, also across
// games whose maps are equal; the reference's metrohash is a third-party package that is not available here, and which
// hash is used only matters for which entries collide).  With one map for all games the key is the state's hash.  The table
// is only READ inside wave_kernel and only WRITTEN by cache_put_kernel between two wave kernels, so no entry is
// ever seen half-written.
// every lane returns the same (hi, lo): position-tagged words mixed per lane, combined across the wavefront
__device__ __forceinline__ void state_hash_wave(const ScsState& st, int lane, uint64_t& hi, uint64_t& lo) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&st);
  uint64_t a = 0, b = 0;
  for (int i = lane; i < (int)(sizeof(ScsState) / 4); i += 64) {
    const uint64_t v = ((uint64_t)(uint32_t)i << 32) | w[i];
    a += mix64(v ^ 0x9e3779b97f4a7c15ull);
    b += mix64(v * 0xd6e8feb86659fd93ull + 0x2545f4914f6cdd1dull);
  }
  for (int o = 32; o; o >>= 1) {
    a += __shfl_xor((unsigned long long)a, o, 64);
    b += __shfl_xor((unsigned long long)b, o, 64);
  }
  hi = mix64(a ^ (b >> 7));
  lo = mix64(b ^ (a << 9));
  if (hi == 0 && lo == 0) lo = 1;                                 // (0, 0) marks an empty entry
}
// the key of game slot g's leaf with state hash (hi, lo): per-game maps mix in the digest of the slot's map row
__device__ __forceinline__ void cache_key_of(const SearchParams& p, int g, uint64_t& hi, uint64_t& lo) {
  if (!p.rules_key) return;                                       // one map: the state's hash as it is
  const uint64_t* const m = p.rules_key + 2 * (size_t)p.rules_row[g];
  const uint64_t a = hi ^ m[0], b = lo ^ m[1];
  hi = mix64(a ^ (b >> 7));
  lo = mix64(b ^ (a << 9));
  if (hi == 0 && lo == 0) lo = 1;
}
__global__ void cache_count_kernel(const uint64_t* __restrict__ c_id, int64_t entries, int64_t* __restrict__ out) {
  long long n = 0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < entries; e += (int64_t)gridDim.x * blockDim.x)
    n += (c_id[2 * e] != 0 || c_id[2 * e + 1] != 0) ? 1 : 0;
  if (n) atomicAdd((unsigned long long*)out, (unsigned long long)n);
}
// After the network: the wave's evaluated leaves go into the table (KeylessCache.put: the newest entry replaces
// what the slot held).  One wavefront per leaf; of two leaves of the same wave that map to the same entry the first
// to arrive writes it, the other is dropped (both are valid values for their keys).
__global__ __launch_bounds__(64) void cache_put_kernel(SearchParams p, const int32_t* __restrict__ n_leaves) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= *n_leaves) return;
  const uint64_t hi = p.leaf_key[2 * slot], lo = p.leaf_key[2 * slot + 1];
  const size_t e = (size_t)(lo & ((1ull << p.c_bits) - 1));
  int old = 0;
  if (lane == 0) old = atomicExch(&p.c_writer[e], p.c_wave);
  old = __shfl(old, 0, 64);
  if (old == p.c_wave) return;
  if (lane == 0) {
    if (p.c_id[2 * e] == 0 && p.c_id[2 * e + 1] == 0) atomicAdd((unsigned long long*)&p.counters[10], 1ull);
    p.c_id[2 * e] = hi;
    p.c_id[2 * e + 1] = lo;
    p.c_value[e] = p.eval_value[slot];
  }
  const int A = p.num_actions;
  for (int i = lane; i < A; i += 64) p.c_probs[e * A + i] = p.eval_probs[(size_t)slot * A + i];
}

// ---- the tree step both search routes run ---------------------------------------------------------------------------
// wave_kernel (a launch per simulation wave) and persist_leader (a move's whole search in one launch) play the same games
// bit for bit, so the steps whose exactness that rests on -- selection with its tie rule and dtypes, expansion with
// numpy's sum and its total == 0 retry, a fresh child's layout, the backup's addition, the leaf's cache key -- are
// written once, here.  Each route keeps what differs: where a level's first 64 children come from (a load / a copy
// fetched under the rule step), where the path lives (memory / a register per lane), when the backup reads the path's
// statistics, where the evaluation comes from.  No helper is told which route called it.

// what a level of the descent needs of the node it leaves
struct Level { int visit, child_base, n_children, to_play; };
__device__ __forceinline__ Level level_of(const SNode& n) { return Level{n.visit, n.child_base, n.n_children, n.to_play}; }

// One level of the descent (Explorer.select_child, :99-112): lane j scores children j, j + 64, ... of the node `par`,
// `first(j)` supplying child j < 64 and the rest loaded here; the wavefront's best (score, action) wins.  Returns the
// winning key (action << 8 | child index), the chosen child's slot in `node` and its Level in `par`.
// One dependent load per level: the chosen child's record was read when it was scored, so the lane that holds it
// hands the four words the next level needs (visit count, first child, children count, to_play) to the wavefront
// (v_readlane: the winner is wave-uniform) instead of every level re-reading its parent from memory.
template <typename First>
__device__ __forceinline__ int select_level(const SearchParams& p, const SNode* nodes, Level& par, double sq, double cb,
                                            int lane, First first, int& node) {
  const bool negate = par.to_play == p.negate_player;
  double score = -INFINITY;
  int key = -1;
  Level best{0, 0, 0, 0};                                        // this lane's best child so far
  for (int j = lane; j < par.n_children; j += 64) {              // one chunk of 64 children per round, usually one
    const SNode c = j < 64 ? first(j) : nodes[par.child_base + j];
    const double sc = child_score(p, c, sq, cb, negate);
    const int ky = ((int)c.action << 8) | j;                     // j < 256; children are in ascending action order
    if (sc > score || (sc == score && ky > key)) {
      score = sc; key = ky;
      best = level_of(c);
    }
  }
  const int my_key = key;
  key = wave_argmax_key(score, key);          // max over (score, action): the larger action wins a tie (Explorer.py:100)
  // the lane that scored the winner (keys are unique: they carry the child index)
  const unsigned long long holders = __ballot(my_key == key);
  const int wl = __builtin_amdgcn_readfirstlane(__ffsll((long long)holders) - 1);
  node = par.child_base + (key & 0xff);
  par = Level{__builtin_amdgcn_readlane(best.visit, wl), __builtin_amdgcn_readlane(best.child_base, wl),
              __builtin_amdgcn_readlane(best.n_children, wl), __builtin_amdgcn_readlane(best.to_play, wl)};
  return key;
}

// The ascending list of the legal actions in a mask (Explorer.py:163-165) into sidx: lane l enumerates mask word
// 64 w + l = `word(w)` (0 past the mask's end) behind a prefix sum of the words' bit counts.  Returns their number.
template <typename Words>
__device__ __forceinline__ int legal_list_of(Words word, int* sidx, int lane) {
  int k = 0;
#pragma unroll
  for (int w = 0; w < (MASK_WORDS + 63) / 64; ++w) {
    uint32_t bits = word(w);
    int inc = __popc(bits);
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    int off = k + inc - __popc(bits);
    while (bits) {
      const int b = __ffs(bits) - 1;
      bits &= bits - 1;
      if (off < MAXC_LIMIT) sidx[off] = (w * 64 + lane) * 32 + b;
      ++off;
    }
    k += __shfl(inc, 63, 64);
  }
  return k;
}

// Expansion (Explorer.py:162-181): child j = the j-th legal action, prior = its masked probability / their float32
// np.sum.  Child 64 c + lane's action is in my_idx[c] (0x7fffffff past the k-th) and its probability in my_val[c] (0
// past the k-th); the records go to nodes[base .. base + k) and `parent` is linked to them.
template <int CH>
__device__ __forceinline__ void expand_children(const SearchParams& p, SNode* nodes, int parent, int base, int k, int lane,
                                                const int (&my_idx)[CH], float (&my_val)[CH]) {
  float total = np_sum_sparse_f32_wave<CH>(p, my_idx, my_val, k);
  if (total == 0.0f) {                  // probs += mask (Explorer.py:171-173)
#pragma unroll
    for (int c = 0; c < CH; ++c) my_val[c] = my_val[c] + 1.0f;
    total = np_sum_sparse_f32_wave<CH>(p, my_idx, my_val, k);
  }
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int j = c * 64 + lane;
    if (j < k) nodes[base + j] = blank_node((double)(my_val[c] / total), my_idx[c]);
  }
  if (lane == 0) {
    nodes[parent].child_base = base;
    nodes[parent].n_children = (uint16_t)k;
  }
}

// backup (Explorer.py:132-135): the same value to every node of the path, root included
__device__ __forceinline__ void backup_node(SNode& n, double v) {
  n.visit += 1;
  n.value_sum = n.value_sum + v;
}
// the path's entries from level `from` on, read from memory: from = 64 behind a first 64 levels that the caller holds in
// registers (one per lane), 0 for the whole path
__device__ __forceinline__ void backup_tail(SNode* nodes, const int32_t* path, int from, int plen, int lane, double v) {
  for (int i = from + lane; i < plen; i += 64) backup_node(nodes[path[i]], v);
}

// the cache key (hi, lo) of game slot g's leaf with scratch state sc; returns the entry its low bits select
__device__ __forceinline__ size_t leaf_cache_key(const SearchParams& p, int g, const ScsState& sc, int lane, uint64_t& hi,
                                                 uint64_t& lo) {
  state_hash_wave(sc, lane, hi, lo);
  cache_key_of(p, g, hi, lo);
  return (size_t)(lo & ((1ull << p.c_bits) - 1));
}
// what probability pr of action i adds to a cache entry's check word (cache_check_word)
__device__ __forceinline__ uint64_t check_term(int i, float pr) {
  return mix64((((uint64_t)(uint32_t)i << 32) | __builtin_bit_cast(uint32_t, pr)) ^ 0x9e3779b97f4a7c15ull);
}

// The per-pass constants of wave_network and what its callers place around a pass: the program's header words (read
// once per move by the caller).
struct WaveNetArgs {
  const Fused16Program* prog;
  int n_ops, rows, H, Wd;
  int solo_at, solo_pol, solo_zero_off, solo_zero_len;
  int in_off, in_cs, pol_off, pol_cs, val_off, val_cs;
};
// the program's header, one dword per lane, handed round by v_readlane
__device__ __forceinline__ WaveNetArgs wave_net_args(const Fused16Program* prog, int lane) {
  const uint32_t hdr = fused16_header_dword(prog, lane);
  return WaveNetArgs{prog, FUSED16_HDR(hdr, n_ops), FUSED16_HDR(hdr, hw), FUSED16_HDR(hdr, h), FUSED16_HDR(hdr, wd),
                     FUSED16_HDR(hdr, solo_at), FUSED16_HDR(hdr, solo_pol), FUSED16_HDR(hdr, solo_zero_off),
                     FUSED16_HDR(hdr, solo_zero_len), FUSED16_HDR(hdr, in_off), FUSED16_HDR(hdr, in_cs), FUSED16_HDR(hdr, pol_off),
                     FUSED16_HDR(hdr, pol_cs), FUSED16_HDR(hdr, val_off), FUSED16_HDR(hdr, val_cs)};
}

// One simulation wave of one game, one wavefront per game (Explorer.run_mcts, :49-61):
//   mode & 1  finish the pending expansion with the supplied evaluation (Explorer.py:162-181) and
//             back its value up           probs [n_leaves][A] float32 post-softmax, value [n_leaves]
//   mode & 2  simulate until the game waits on a leaf that needs an evaluation, its simulations
//             are used up, or `budget` simulations that ended in terminal leaves have run
// The rules, the scratch game and the legal-move mask live in LDS: the rules run on lane 0
// (serial, latency-bound code), the children are scored, the mask and the state image are built
// and the new children are written by all lanes.
__global__ __launch_bounds__(64) void wave_kernel(SearchParams p, int mode, const float* __restrict__ probs,
                                                   const float* __restrict__ value, float* __restrict__ images,
                                                   int32_t* __restrict__ leaf_game) {
  __shared__ __attribute__((aligned(16))) ScsRules R;
  __shared__ ScsState sc;
  __shared__ uint32_t smask[MASK_WORDS];
  __shared__ int sidx[MAXC_LIMIT];
  const int g = blockIdx.x;
  const int lane = lane_id();
#ifdef NZ_SCS_STAMPS     // diagnostic build: where a game's wave time goes (nz_scs_search_phase_ticks)
  unsigned long long tk[6] = {0, 0, 0, 0, 0, 0}, ts = __builtin_amdgcn_s_memtime();
#define NZ_STAMP(slot) { const unsigned long long now = __builtin_amdgcn_s_memtime(); tk[slot] += now - ts; ts = now; }
#else
#define NZ_STAMP(slot)
#endif
  if (g == 0 && lane == 0 && p.clear_counters != nullptr) { p.clear_counters[0] = 0; p.clear_counters[1] = 0; p.clear_counters[2] = 0; }
  // everything this wave needs from the game's records in ONE round of loads (a chain of dependent loads, each
  // behind the branch on the previous one, costs a memory round trip per link)
  const uint32_t* m = p.leaf_mask + (size_t)g * MASK_WORDS;
  int32_t* path = p.path + (size_t)g * p.max_path;
  const int terminal = p.real[g].terminal;
  const int pend = p.pending[g];
  const int plen_in = p.path_len[g];
  const int base_in = p.node_count[g];
  const int sims_in = p.sims_left[g];
  const int root = p.root[g];
  uint32_t mword[(MASK_WORDS + 63) / 64];
#pragma unroll
  for (int w = 0; w < (MASK_WORDS + 63) / 64; ++w) mword[w] = w * 64 + lane < MASK_WORDS ? m[w * 64 + lane] : 0u;
  const int my_path0 = path[lane];                     // max_path > 64
  if (terminal) return;
  const int A = p.num_actions;
  SNode* nodes = arena(p, g);

  const bool expanding = (mode & 1) && pend >= 0;
  if (expanding) {
    const int slot = pend;
    const int plen = plen_in;
    const int leaf = plen <= 64 ? __shfl(my_path0, plen - 1, 64) : path[plen - 1];
    // second round: the evaluation and the path's statistics
    const double v = (double)value[slot];
    const int my_node = lane < plen ? my_path0 : 0;
    const int my_visit = lane < plen ? nodes[my_node].visit : 0;
    const double my_vs = lane < plen ? nodes[my_node].value_sum : 0.0;
    const int k = legal_list_of([&](int w) { return mword[w]; }, sidx, lane);
    const int base = base_in;
    const bool overflow = k > p.maxc;
    if (overflow || base + k > p.half_cap) {
      if (lane == 0) atomicOr(p.error_flag, overflow ? 16 : 1);
    } else {
      __syncthreads();
      int my_idx[MAXC_CHUNKS];                // child 64 c + lane: its action and its masked probability
      float my_val[MAXC_CHUNKS];
#pragma unroll
      for (int c = 0; c < MAXC_CHUNKS; ++c) {
        const int j = c * 64 + lane;
        my_idx[c] = j < k ? sidx[j] : 0x7fffffff;
        my_val[c] = j < k ? probs[(size_t)slot * A + my_idx[c]] : 0.0f;
      }
      expand_children<MAXC_CHUNKS>(p, nodes, leaf, base, k, lane, my_idx, my_val);
      if (lane == 0) p.node_count[g] = base + k;
    }
    if (lane == 0) {
      p.pending[g] = -1;
      p.sims_left[g] = sims_in - 1;
    }
    // backup (Explorer.py:132-135): the path's statistics were read above; the leaf's new children do not touch them
    if (lane < plen) {
      nodes[my_node].visit = my_visit + 1;
      nodes[my_node].value_sum = my_vs + v;
    }
    backup_tail(nodes, path, 64, plen, lane, v);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  NZ_STAMP(0);                                  // expansion + backup of the evaluated leaf
  // The run's simulation / expansion counters take ONE atomic each per game and wave, as the wavefront leaves: a thousand
  // games add to the same two words, and an atomic still on its way holds up every later wait for a load (vmcnt counts
  // in order) -- the descent's first node reads stood behind the expansion's.
  const unsigned long long n_expanded = expanding ? 1ull : 0ull;
  auto leave = [&](unsigned long long sims_done) {
    if (lane == 0) {
      if (sims_done) atomicAdd((unsigned long long*)&p.counters[0], sims_done);
      if (n_expanded) atomicAdd((unsigned long long*)&p.counters[1], n_expanded);
    }
  };
  if (!(mode & 2) || (pend >= 0 && !expanding)) { leave(n_expanded); return; }
  int sims_left = expanding ? sims_in - 1 : sims_in;
  if (sims_left <= 0) { leave(n_expanded); return; }

  {   // rules -> LDS: 16 bytes per lane and load, all loads in flight before the first store
    static_assert(sizeof(ScsRules) % 4 == 0 && sizeof(ScsState) % 4 == 0, "copied as dwords");
    constexpr int N16 = (int)(sizeof(ScsRules) / 16), PER_LANE = (N16 + 63) / 64;
    const ScsRules* const my_rules = &rules_of(p, g);
    const uint4* src = reinterpret_cast<const uint4*>(my_rules);
    uint4* dst = reinterpret_cast<uint4*>(&R);
    uint4 tmp[PER_LANE];
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j)
      if (j * 64 + lane < N16) tmp[j] = src[j * 64 + lane];
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j)
      if (j * 64 + lane < N16) dst[j * 64 + lane] = tmp[j];
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(my_rules);
    uint32_t* d4 = reinterpret_cast<uint32_t*>(&R);
    for (int i = N16 * 4 + lane; i < (int)(sizeof(ScsRules) / 4); i += 64) d4[i] = s4[i];
  }
  NZ_STAMP(1);                                  // rules -> LDS
  long n_sim = 0;
  int budget = p.terminal_budget;
  bool queued = false;

  while (sims_left > 0 && budget > 0) {
    {   // scratch_game = game.shallow_clone()
      const uint32_t* src = reinterpret_cast<const uint32_t*>(&p.real[g]);
      uint32_t* dst = reinterpret_cast<uint32_t*>(&sc);
      for (int i = lane; i < (int)(sizeof(ScsState) / 4); i += 64) dst[i] = src[i];
      __syncthreads();
    }
    NZ_STAMP(2);                                // scratch game = real game
    int node = root, plen = 1;
    if (lane == 0) path[0] = root;
    bool bad = false;
    Level par = level_of(nodes[root]);
    while (par.n_children > 0) {
      if (par.visit >= p.tab_len || plen >= p.max_path) { bad = true; break; }
      const double sq = p.sqrt_tab[par.visit], cb = p.bias_tab[par.visit];
      const int key = select_level(p, nodes, par, sq, cb, lane, [&](int j) { return nodes[par.child_base + j]; }, node);
      if (lane == 0) path[plen] = node;
      scs_step_wave(R, sc, key >> 8, lane);
      ++plen;
    }
    if (bad) {
      if (lane == 0) atomicOr(p.error_flag, 2);
      sims_left = 0;
      break;
    }
    __syncthreads();                          // lane 0's steps on the scratch game are visible to every lane
    NZ_STAMP(3);                                // descent: scores, argmax, rule steps
    // evaluate (Explorer.py:137-181)
    const int to_play = sc.player, term = sc.terminal;
    if (term) {
      if (lane == 0) {
        nodes[node].to_play = (int8_t)to_play;
        nodes[node].terminal = 1;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      const double v = (double)sc.terminal_value;
      backup_tail(nodes, path, 0, plen, lane, v);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      --sims_left;
      --budget;
      ++n_sim;
      continue;
    }
    // leaf needs an evaluation: from the cache if its state is there (Explorer.py:147-149), else queue its state
    // image for the network; either way remember its legal actions for the expansion at the start of the next wave
    uint64_t key_hi = 0, key_lo = 0;
    bool hit = false;
    size_t entry = 0;
    if (p.c_bits > 0) {
      entry = leaf_cache_key(p, g, sc, lane, key_hi, key_lo);
      hit = p.c_id[2 * entry] == key_hi && p.c_id[2 * entry + 1] == key_lo;      // uniform: every lane reads the same words
    }
    int slot = 0;
    if (lane == 0) {
      if (hit) {
        slot = p.c_hit_base + atomicAdd(p.hit_count, 1);
        atomicAdd((unsigned long long*)&p.counters[8], 1ull);
      } else {
        slot = atomicAdd(p.leaf_count, 1);
        leaf_game[slot] = g;
        if (p.c_bits > 0) {
          p.leaf_key[2 * slot] = key_hi;
          p.leaf_key[2 * slot + 1] = key_lo;
          atomicAdd((unsigned long long*)&p.counters[9], 1ull);
        }
      }
      p.pending[g] = slot;
      p.path_len[g] = plen;
      nodes[node].to_play = (int8_t)to_play;
    }
    slot = __shfl(slot, 0, 64);
    scs_legal_mask_wave<MASK_WORDS>(R, sc, smask, lane);
    uint32_t* m = p.leaf_mask + (size_t)g * MASK_WORDS;
    for (int i = lane; i < MASK_WORDS; i += 64) m[i] = smask[i];
    if (hit) {                                  // the cached evaluation takes the place of the network's
      for (int i = lane; i < A; i += 64) p.eval_probs[(size_t)slot * A + i] = p.c_probs[entry * A + i];
      if (lane == 0) p.eval_value[slot] = p.c_value[entry];
      queued = true;
      NZ_STAMP(4);
      break;
    }
    if (p.image_row_stride > 0)       // straight into the network's input rows: group of 16 slots, then cell, then slot
      scs_state_image_wave<true>(R, sc, images + ((size_t)(slot >> 4) * R.tiles * 16 + (slot & 15)) * p.image_row_stride,
                                 p.image_row_stride, lane);
    else
      scs_state_image_wave<false>(R, sc, images + (size_t)slot * R.channels * R.tiles, 0, lane);
    queued = true;
    NZ_STAMP(4);                                // legal mask + state image of the queued leaf
    break;
  }
  NZ_STAMP(5);                                  // terminal-leaf simulations
#ifdef NZ_SCS_STAMPS
  if (lane == 0)
    for (int i = 0; i < 6; ++i) atomicAdd((unsigned long long*)&p.counters[2 + i], tk[i]);
#endif
  if (lane == 0) {
    p.sims_left[g] = sims_left;
    if (queued || sims_left > 0) atomicAdd(p.active_count, 1);
  }
  leave((unsigned long long)n_sim + n_expanded);
}


// ---- persistent self-play: one wavefront per game, the whole move's search in one launch --------------------------------
// wave_kernel + a network launch per simulation make every game wait for the slowest of all games, a thousand times a
// move.  Here a game's wavefront runs its simulations on its own (Explorer.run_mcts, :49-61: one in flight per tree):
// descent and rules as in wave_kernel, then the NETWORK FOR ITS OWN LEAF -- the split-bf16 arithmetic of
// fused16_net_kernel (boardnet.hip) for one position: 25 cells = two row tiles, every layer's weights streamed from L2,
// activations in the wavefront's own block of LDS -- softmax, expansion, backup, next simulation.  No barrier, no other
// game, no host until the move's simulations are used up.  Four games (wavefronts) per workgroup share the rules block.
// A network handle in the plain-bf16 mode (nz_boardnet_precision) runs the PREC_BF16 instantiation: the same pass on one
// rounded bf16 per number (fused16_dev.hpp), one pair of MFMAs per K step; the search around it is the same code.
struct PersistArgs {
  const Fused16Program* prog;
  int32_t net_floats, stage_off, stage_floats, inp, in_channels;
  int32_t wave_bytes;             // a game's LDS block: real game, scratch game, legal mask, legal list, flags, network
  int32_t rules_per_game;         // 1: every game slot keeps its own description in LDS (per-game maps), 0: one for the workgroup
  // leaf evaluations of chosen games, for the oracle replay of tests/scs_replay.py (null: none)
  const int32_t* rec_slot;        // [G] slot or -1
  int32_t rec_cap;
  int32_t* rec_count;             // [slots]
  uint64_t* rec_digest;           // [slots][cap][2] image_hash_wave of the leaf's float32 planes
  float* rec_probs;               // [slots][cap][A]
  float* rec_value;               // [slots][cap]
};
constexpr int PERSIST_GAMES = 4;                 // games per workgroup
constexpr int PERSIST_WAVES = 2 * PERSIST_GAMES;  // a leader and a helper wavefront per game
constexpr int PERSIST_THREADS = PERSIST_WAVES * 64;
constexpr int PERSIST_FLAG_BYTES = 32;           // per game: the step numbers of its (up to four) wavefronts, the pass number / exit word
constexpr int PERSIST_EXIT = 0x7fffffff;
constexpr int PERSIST_STATE_BYTES = (int)((sizeof(ScsState) + 15) / 16 * 16);
constexpr int PERSIST_MASK_BYTES = (MASK_WORDS * 4 + 15) / 16 * 16;
constexpr int PERSIST_GAME_BYTES = 2 * PERSIST_STATE_BYTES + PERSIST_MASK_BYTES + MAXC_LIMIT * 4 + PERSIST_FLAG_BYTES;
constexpr int PERSIST_RULES_BYTES = (int)((sizeof(ScsRules) + 15) / 16 * 16);
typedef const __attribute__((address_space(1))) u32x4* gptr4u;

// 128-bit digest of a leaf's float32 planes [channels][tiles] as they sit in the staging rows ([tile][inp])
__device__ __forceinline__ void image_hash_wave(const float* stage, int inp, int channels, int tiles, int lane, uint64_t& hi, uint64_t& lo) {
  scs_image_digest_wave([&](int c, int t) { return stage[t * inp + c]; }, channels, tiles, lane, hi, lo);
}

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
// the check word of a cache entry: per-lane sums of per-probability mixes (acc), the value and the key
__device__ __forceinline__ uint64_t cache_check_word(uint64_t acc, float value, uint64_t key_hi, uint64_t key_lo) {
  for (int o = 32; o; o >>= 1) acc += __shfl_xor((unsigned long long)acc, o, 64);
  return mix64(acc ^ mix64(key_hi ^ (uint64_t)__builtin_bit_cast(uint32_t, value)) ^ (key_lo * 0xd6e8feb86659fd93ull));
}

// One conv layer's K loop for one position and ONE column tile: both row tiles (25 cells), NTAPS x KGT steps as
// straight-line code.  Activations (the MFMA's second operand) come from LDS, this lane's operand row per tap in srow,
// read one step ahead of the MFMAs that use them; the weights (first operand) straight from the packed L2 stream, their
// loads running AHEAD steps in front (an L2 round trip is several steps long; three or six steps measured no faster,
// DESIGN §5c).
constexpr int WAVE_AHEAD = 2;
// The plain-bf16 mode (PREC = PREC_BF16, fused16_dev.hpp): a step is one pair of MFMAs, a sixth of the float32 mode's, so
// the weights run six steps ahead to stay the same time in front; a step's weights are one piece (1 KB of the stream).
constexpr int WAVE_AHEAD_BF16 = 6;
template <int PREC> constexpr int wave_ahead() { return PREC == PREC_BF16 ? WAVE_AHEAD_BF16 : WAVE_AHEAD; }
#ifndef NZ_PERSIST_SYNC_DRAIN
#define NZ_PERSIST_SYNC_DRAIN 0   // 1: a meeting waits for this wavefront's LDS stores before it posts its number
#endif
// the first WAVE_AHEAD steps' weights of a column tile's stream (steps are contiguous whatever the layer's K groups)
// (buffer loads: a wave-uniform descriptor of the column tile's stream, ONE vector register with this lane's byte offset,
// the step's offset as a scalar -- plain global loads keep a 64-bit address pair alive per load in flight, forty registers)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wave_weights_rsrc(const uint32_t* wg, int chunks16) {
  // (pinned to scalar registers: taken for lane-dependent, the descriptor makes every load of the stream a loop over
  // the lanes' values -- seen once, a fifth of the round)
  const uint64_t a = (uint64_t)(uintptr_t)wg;
  const uint64_t u = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<uint32_t*>((uintptr_t)u), (short)0,
                                           __builtin_amdgcn_readfirstlane(chunks16 * 16), 0x00020000);
}
// one step's three pieces; the stream position is ONE running vector register (the step's 3 KB added after its loads, the
// pieces as immediate offsets): a scalar offset per (step, piece) was forty scalar registers of constants held across
// the whole pass, and the layer's own scalars went to spill lanes for them
template <int NP>
__device__ __forceinline__ void wave_weights_step(u32x4 (&dst)[NP], __amdgpu_buffer_rsrc_t rs, int& wv) {
#pragma unroll
  for (int piece = 0; piece < NP; ++piece)
    dst[piece] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, wv + piece * 1024, 0, 0));
  wv += NP * 1024;
  asm volatile("" : "+v"(wv));
}
template <int AHEAD, int NP>
__device__ __forceinline__ void wave_weights_prologue(u32x4 (&bq)[AHEAD + 1][NP], __amdgpu_buffer_rsrc_t rs, int& wv, int lane) {
  wv = lane * 16;
  asm volatile("" : "+v"(wv));
#pragma unroll
  for (int st = 0; st < AHEAD; ++st) wave_weights_step(bq[st], rs, wv);
}
// Pieces buffers in a game's LDS block: [row][32-channel group][piece][four 16-byte chunks], a row every `cs` floats
// (48 per group, + 16 when the groups are even in number: rows 256 bytes apart would share their banks), chunk q of row
// r at position q ^ ((r >> 2) & 3).  A K step's operand reads are then ONE address per (row tile, tap) -- made once per
// layer -- plus immediates (group x 192 + piece x 64 bytes): no address arithmetic between the MFMAs, whose gaps hide
// eight cycles of other vector issue each and no more.
constexpr int PIECE_FLOATS = 16, GROUP_FLOATS = 3 * PIECE_FLOATS;
typedef const __attribute__((address_space(3))) u32x4* lds_u32x4;
// this lane's operand rows of a position's conv taps, a byte per tap (four taps to a register): the row index (rows = the
// buffers' row of zeros) in rows[], the byte offset of this lane's chunk within a 32-channel group of that row in swz[]
template <int NTAPS>
struct TapRows {
  static constexpr int WORDS = (NTAPS + 3) / 4;
  uint32_t rows[WORDS], swz[WORDS];
  __device__ __forceinline__ uint32_t row(int tap) const { return (rows[tap >> 2] >> ((tap & 3) * 8)) & 0xffu; }
  __device__ __forceinline__ uint32_t chunk(int tap) const { return (swz[tap >> 2] >> ((tap & 3) * 8)) & 0xffu; }
};
template <bool HEX, int NTAPS>
__device__ __forceinline__ void wave_tap_rows(TapRows<NTAPS>& t, int row, int rows, int H, int Wd, int lane) {
  const bool row_ok = row < rows;
  const int cy = row / Wd, cx = row - cy * Wd;
#pragma unroll
  for (int w = 0; w < TapRows<NTAPS>::WORDS; ++w) { t.rows[w] = 0u; t.swz[w] = 0u; }
#pragma unroll
  for (int tap = 0; tap < NTAPS; ++tap) {
    const int dy = tap_dy<HEX>(tap, cx), dx = tap_dx<HEX>(tap);
    const bool on = row_ok && (unsigned)(cy + dy) < (unsigned)H && (unsigned)(cx + dx) < (unsigned)Wd;
    const int r = on ? row + dy * Wd + dx : rows;       // (row index `rows`: every buffer's row of zeros)
    t.rows[tap >> 2] |= (uint32_t)r << ((tap & 3) * 8);
    t.swz[tap >> 2] |= (uint32_t)(((lane >> 4) ^ ((r >> 2) & 3)) << 4) << ((tap & 3) * 8);
  }
}

template <int NTAPS, int KGT, int RT = 2, int PREC = PREC_F32>
__device__ __forceinline__ void wave_conv(f32x4 (&acc)[RT], const TapRows<NTAPS> (&srow)[RT], uint32_t src, uint32_t cs4,
                                          __amdgpu_buffer_rsrc_t wrs, int& wv, u32x4 (&bq)[wave_ahead<PREC>() + 1][prec_pieces(PREC)],
                                          unsigned long long* tkn = nullptr, unsigned long long* tsn = nullptr) {
  constexpr int STEPS = NTAPS * KGT;
  constexpr int AHEAD = wave_ahead<PREC>();
  constexpr int NP = prec_pieces(PREC);
  static_assert(STEPS >= AHEAD, "the prologue is always AHEAD steps");
  u32x4 a[2][RT][NP];
  // a tap's operand address: source buffer + row x row stride + this lane's chunk (LDS byte address); two taps' worth are
  // alive at a time
  uint32_t ad[2][RT];
  auto address = [&](int tap) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) ad[tap & 1][rt] = __umul24(srow[rt].row(tap), cs4) + srow[rt].chunk(tap) + src;
  };
  auto read = [&](int st, int rt, int piece) -> u32x4 {
    const int tap = st / KGT, kg = st - tap * KGT;
    return *reinterpret_cast<lds_u32x4>(ad[tap & 1][rt] + (uint32_t)((kg * GROUP_FLOATS + piece * PIECE_FLOATS) * 4));
  };
  address(0);
#pragma unroll
  for (int piece = 0; piece < NP; ++piece)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) a[0][rt][piece] = read(0, rt, piece);
  if (STEPS > 1 && 1 / KGT != 0) address(1 / KGT);
#ifdef NZ_PERSIST_HEADSTAMP   // diagnostic: how long a layer waits for its first operands (slot 3; perturbs the pipeline)
  if (tkn) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const unsigned long long now = __builtin_amdgcn_s_memtime();
    tkn[3] += now - *tsn;
    *tsn = now;
  }
#endif
  if constexpr (RT == 2 && PREC == PREC_BF16) {
    // The plain-bf16 step: ONE pair of MFMAs (row tile 0, row tile 1) on piece plane 0, in the float32 mode's step order.
    // Its two slots: behind the first MFMA the next step's operand read for row tile 0 and the weights of AHEAD steps on,
    // behind the second the read for row tile 1 and the address of the tap after next.
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const bool more = st + 1 < STEPS;
      __builtin_amdgcn_sched_barrier(0);
      acc[0] = mfma_bf16(bq[st % (AHEAD + 1)][0], a[st & 1][0][0], acc[0]);
      if (more) a[(st + 1) & 1][0][0] = read(st + 1, 0, 0);
      if (st + AHEAD < STEPS) wave_weights_step(bq[(st + AHEAD) % (AHEAD + 1)], wrs, wv);
      __builtin_amdgcn_sched_barrier(0);
      acc[1] = mfma_bf16(bq[st % (AHEAD + 1)][0], a[st & 1][1][0], acc[1]);
      if (more) a[(st + 1) & 1][1][0] = read(st + 1, 1, 0);
      if (st + 2 < STEPS && (st + 2) / KGT != (st + 1) / KGT) address((st + 2) / KGT);
      __builtin_amdgcn_sched_barrier(0);
    }
  } else if constexpr (RT == 2) {
    // A step as six SLOTS, each one pair of MFMAs (row tile 0, row tile 1; step16's term order) with loads in its shadow
    // (an MFMA's gap hides eight cycles of other vector issue, no more): slots 0..2 the next step's operand reads in the
    // order the next step's pairs want them (pieces 1, 2, 0: every read has a whole step to arrive), slot 3 the weights of
    // AHEAD steps on, slot 4 the address of the tap after next.  Scheduling barriers between the slots: left to itself
    // the scheduler put the reads behind the step's MFMAs (their latency at the head of every step); given load slots
    // only, it ran each row tile's six MFMAs as one dependent chain.
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const bool more = st + 1 < STEPS;
      const u32x4 (&b)[3] = bq[st % (AHEAD + 1)];
      const u32x4 (&a0)[3] = a[st & 1][0];
      const u32x4 (&a1)[3] = a[st & 1][1];
      u32x4 (&n0)[3] = a[(st + 1) & 1][0];
      u32x4 (&n1)[3] = a[(st + 1) & 1][1];
      u32x4 (&nb)[3] = bq[(st + AHEAD) % (AHEAD + 1)];
#define NZ_PAIR(B, A)                         \
  acc[0] = mfma_bf16(b[B], a0[A], acc[0]);    \
  acc[1] = mfma_bf16(b[B], a1[A], acc[1]);
      __builtin_amdgcn_sched_barrier(0);
      NZ_PAIR(1, 1)
      if (more) { n0[1] = read(st + 1, 0, 1); n1[1] = read(st + 1, 1, 1); }
      __builtin_amdgcn_sched_barrier(0);
      NZ_PAIR(0, 2)
      if (more) { n0[2] = read(st + 1, 0, 2); n1[2] = read(st + 1, 1, 2); }
      __builtin_amdgcn_sched_barrier(0);
      NZ_PAIR(2, 0)
      if (more) { n0[0] = read(st + 1, 0, 0); n1[0] = read(st + 1, 1, 0); }
      __builtin_amdgcn_sched_barrier(0);
      NZ_PAIR(0, 1)
      if (st + AHEAD < STEPS) wave_weights_step(nb, wrs, wv);
      __builtin_amdgcn_sched_barrier(0);
      NZ_PAIR(1, 0)
      if (st + 2 < STEPS && (st + 2) / KGT != (st + 1) / KGT) address((st + 2) / KGT);
      __builtin_amdgcn_sched_barrier(0);
      NZ_PAIR(0, 0)
      __builtin_amdgcn_sched_barrier(0);
#undef NZ_PAIR
    }
  } else {
    // one row tile (an odd last column tile): the next step's reads and weights, then the step's six MFMAs
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      if (st + 1 < STEPS) {
#pragma unroll
        for (int piece = 0; piece < NP; ++piece)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) a[(st + 1) & 1][rt][piece] = read(st + 1, rt, piece);
      }
      if (st + AHEAD < STEPS) wave_weights_step(bq[(st + AHEAD) % (AHEAD + 1)], wrs, wv);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        if constexpr (PREC == PREC_BF16) step16_bf16(acc[rt], a[st & 1][rt][0], bq[st % (AHEAD + 1)][0]);
        else step16(acc[rt], a[st & 1][rt], bq[st % (AHEAD + 1)]);
      }
      if (st + 2 < STEPS && (st + 2) / KGT != (st + 1) / KGT) address((st + 2) / KGT);
      __builtin_amdgcn_sched_barrier(0);          // (the scheduler would hoist every later step's loads up here: spills)
    }
  }
}

// float offset of (row, channel c0 = 16 ct + 4 (lane >> 4)) within a pieces buffer's row, piece 0
__device__ __forceinline__ int pieces_chunk(int ct, int lane, int row) {
  return (ct >> 1) * GROUP_FLOATS + (((((ct & 1) << 1) | (lane >> 5)) ^ ((row >> 2) & 3)) << 2) + ((lane >> 4) & 1) * 2;
}

// A layer's epilogue for one tile: residual, activation, split into pieces (or float32 rows), store.  The values are
// fused16_dev.hpp's epi16_* (fused16_net_kernel calls the same); the addresses are this layout's.
template <int PREC = PREC_F32>
__device__ __forceinline__ void wave_epilogue(const f32x4& acc, float* __restrict__ net, const Fused16Op& op, int rt, int ct,
                                              int lane, int rows) {
  const int orow = rt * 16 + (lane & 15), c0 = ct * 16 + (lane >> 4) * 4;
  if (orow >= rows) return;
  const int chunk = pieces_chunk(ct, lane, orow);
  float v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = acc[r];
  if (op.offr >= 0) {
    const float* rp = net + op.offr + orow * op.csr + chunk;
    if constexpr (PREC == PREC_BF16) epi16_add_residual_bf16(v, *reinterpret_cast<const uint2*>(rp));
    else {
      const uint2 q0 = *reinterpret_cast<const uint2*>(rp), q1 = *reinterpret_cast<const uint2*>(rp + PIECE_FLOATS),
                  q2 = *reinterpret_cast<const uint2*>(rp + 2 * PIECE_FLOATS);
      epi16_add_residual(v, q0, q1, q2);
    }
  }
  epi16_activate<4>(v, op.act);
  if (op.psd == 0) {
    *reinterpret_cast<f32x4*>(net + op.offd + orow * op.csd + c0) = f32x4{v[0], v[1], v[2], v[3]};
  } else if constexpr (PREC == PREC_BF16) {
    *reinterpret_cast<uint2*>(net + op.offd + orow * op.csd + chunk) = epi16_round(v);
  } else {
    uint2 q[3];
    epi16_split(v, q);
    float* dp = net + op.offd + orow * op.csd + chunk;
#pragma unroll
    for (int piece = 0; piece < 3; ++piece) *reinterpret_cast<uint2*>(dp + piece * PIECE_FLOATS) = q[piece];
  }
}

// wave_epilogue for both row tiles of a column tile at once: the eight values go through every step together (one
// wave-uniform switch, independent chains the scheduler interleaves), the residual reads and the stores are predicated
// per row tile.  (Kept beside wave_epilogue: one template over the number of row tiles cost the persistent kernel 1.4 %,
// profiles/r09_fused16_shared.txt.)
template <int PREC = PREC_F32>
__device__ __forceinline__ void wave_epilogue2(const f32x4 (&acc)[2], float* __restrict__ net, const Fused16Op& op, int ct,
                                               int lane, int rows) {
  const int c0 = ct * 16 + (lane >> 4) * 4;
  int orow[2], chunk[2];
  bool ok[2];
  float v[2][4];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    orow[rt] = rt * 16 + (lane & 15);
    ok[rt] = orow[rt] < rows;
    chunk[rt] = pieces_chunk(ct, lane, orow[rt]);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[rt][r] = acc[rt][r];
  }
  if (op.offr >= 0) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      if (ok[rt]) {
        const float* rp = net + op.offr + orow[rt] * op.csr + chunk[rt];
        if constexpr (PREC == PREC_BF16) epi16_add_residual_bf16(v[rt], *reinterpret_cast<const uint2*>(rp));
        else {
          const uint2 q0 = *reinterpret_cast<const uint2*>(rp), q1 = *reinterpret_cast<const uint2*>(rp + PIECE_FLOATS),
                      q2 = *reinterpret_cast<const uint2*>(rp + 2 * PIECE_FLOATS);
          epi16_add_residual(v[rt], q0, q1, q2);
        }
      }
    }
  }
  epi16_activate<8>(&v[0][0], op.act);
  if (op.psd == 0) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
      if (ok[rt]) *reinterpret_cast<f32x4*>(net + op.offd + orow[rt] * op.csd + c0) = f32x4{v[rt][0], v[rt][1], v[rt][2], v[rt][3]};
    return;
  }
  if constexpr (PREC == PREC_BF16) {           // one rounded piece per row tile, into plane 0
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
      if (ok[rt]) *reinterpret_cast<uint2*>(net + op.offd + orow[rt] * op.csd + chunk[rt]) = epi16_round(v[rt]);
    return;
  }
  uint2 q[2][3];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) epi16_split(v[rt], q[rt]);
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    if (ok[rt]) {
      float* dp = net + op.offd + orow[rt] * op.csd + chunk[rt];
#pragma unroll
      for (int piece = 0; piece < 3; ++piece) *reinterpret_cast<uint2*>(dp + piece * PIECE_FLOATS) = q[rt][piece];
    }
  }
}

template <int NTAPS, int KGT, int RT = 2, int PREC = PREC_F32>
__device__ __forceinline__ void wave_layer_kloop(f32x4 (&acc)[RT], const float* __restrict__ net, const Fused16Op& op,
                                                 const TapRows<NTAPS> (&srow)[RT], int ct, int lane,
                                                 u32x4 (&bq)[wave_ahead<PREC>() + 1][prec_pieces(PREC)], int& wv,
                                                 unsigned long long* tkn = nullptr, unsigned long long* tsn = nullptr) {
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint32_t src = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)(net + op.off0);
  const uint32_t cs4 = (uint32_t)op.cs0 * 4u;
  const __amdgpu_buffer_rsrc_t wrs = wave_weights_rsrc(op.w + (size_t)ct * op.w_chunks * 4, op.w_chunks);
  wave_conv<NTAPS, KGT, RT, PREC>(acc, srow, src, cs4, wrs, wv, bq, tkn, tsn);
}

// The two wavefronts of a game meet (the leader runs the tree and half of every layer, the helper the other half): each
// posts the number of the step it has finished and waits for the other's.  LDS stores of one wavefront reach LDS in
// order, so the partner that sees the number sees the activations stored before it.
__device__ __forceinline__ void pair_sync(int* flags, int me, int& seq, int lane) {
  ++seq;
#if NZ_PERSIST_SYNC_DRAIN
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");      // (LDS only: everything a pair shares is in LDS)
#else
  // (no wait for the stores: the LDS takes one wavefront's operations in the order they were issued, so the number
  // lands behind the activations; the compiler is told not to move them)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#endif
  if (lane == 0) __hip_atomic_store(&flags[me], seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  while (__hip_atomic_load(&flags[me ^ 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < seq) {}
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// every layer of the network for the position whose input pieces sit in the game's block: this wavefront takes the
// column tiles half, half + 2, ... of each layer
#ifdef NZ_PERSIST_STAMPS
#define WSTAMP(slot) { if (tkn) { const unsigned long long now = __builtin_amdgcn_s_memtime(); tkn[slot] += now - tsn; tsn = now; } }
#else
#define WSTAMP(slot)
#endif
// Every layer of the network for the position whose input pieces sit in the game's block.  Trunk layers: this wavefront
// takes column tiles half, half + 2, ... of the layer's PAIRS of column tiles (both row tiles each), then row tile `half`
// of an odd last column tile (whole it was the leader's alone and the helper waited), and the pair meets after every
// layer.  Head layers (from solo_at on): the leader runs the policy head's chain, the helper the value head's, every tile
// of every layer, with no meeting -- the CALLER holds the last one (the leader after its softmax, which needs the
// logits only).
template <bool HEX, int PREC = PREC_F32>
__device__ __forceinline__ void wave_network(const WaveNetArgs& wn, float* __restrict__ net, int lane, int half, int* flags, int& seq,
                                             unsigned long long* tkn = nullptr) {
  unsigned long long tsn = 0;                  // (the stamps' clock; tkn is null outside the diagnostic builds)
#ifdef NZ_PERSIST_STAMPS
  tsn = __builtin_amdgcn_s_memtime();
#endif
  constexpr int ntaps = tap_count<HEX>();
  const int n_ops = wn.n_ops, rows = wn.rows;
  TapRows<ntaps> srow[2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) wave_tap_rows<HEX, ntaps>(srow[rt], rt * 16 + (lane & 15), rows, wn.H, wn.Wd, lane);
  // this wavefront's layers in order: the shared ones, then its own chain
  const int solo_at = wn.solo_at < n_ops ? wn.solo_at : n_ops;
  const int chain_first = half == 0 ? solo_at : solo_at + wn.solo_pol;
  const int chain_len = solo_at < n_ops ? (half == 0 ? wn.solo_pol : n_ops - solo_at - wn.solo_pol) : 0;
  const int n_mine = solo_at + chain_len;
  auto layer_at = [&](int i) { return i < solo_at ? i : chain_first + (i - solo_at); };
  // A layer's descriptor stays in ONE vector register (a dword per lane, fetched a layer ahead) until the layer starts:
  // unpacked a layer early its fields were scalar registers the K loop had no room for (spilled to lanes and back).
  uint32_t cur = n_mine > 0 ? fused16_op_dword(wn.prog, layer_at(0), lane) : 0u;
  uint32_t nxt = n_mine > 1 ? fused16_op_dword(wn.prog, layer_at(1), lane) : 0u;
  int wv = 0;
  u32x4 bq[wave_ahead<PREC>() + 1][prec_pieces(PREC)];
  auto job_weights = [&](const Fused16Op& x, int ct) {
    wave_weights_prologue<wave_ahead<PREC>()>(bq, wave_weights_rsrc(x.w + (size_t)ct * x.w_chunks * 4, x.w_chunks), wv, lane);
  };
  for (int i = 0; i < n_mine; ++i) {
    const Fused16Op op = fused16_unpack(cur);
    cur = nxt;
    if (i + 2 < n_mine) nxt = fused16_op_dword(wn.prog, layer_at(i + 2), lane);
    const int kgt = op.kg0;
    const bool shared = i < solo_at;
    if (i == solo_at && half == 0 && lane * 4 < wn.solo_zero_len)       // (the policy head's hidden buffer: its row of zeros)
      *reinterpret_cast<f32x4*>(net + wn.solo_zero_off + lane * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    const int pair_tiles = shared ? op.ntiles & ~1 : op.ntiles;
    const bool odd = shared && (op.ntiles & 1);
    for (int ct = shared ? half : 0; ct < pair_tiles; ct += shared ? 2 : 1) {
      f32x4 acc[2];
      WSTAMP(4);                    // (the layer's header: descriptor words, addresses)
      job_weights(op, ct);
      for_kgroups(kgt, [&](auto kg) { wave_layer_kloop<ntaps, decltype(kg)::value, 2, PREC>(acc, net, op, srow, ct, lane, bq, wv, tkn, &tsn); });
      WSTAMP(0);
      wave_epilogue2<PREC>(acc, net, op, ct, lane, rows);
      WSTAMP(1);
    }
    if (odd) {
      const int ct = op.ntiles - 1;
      TapRows<ntaps> srow1[1];
#pragma unroll
      for (int w = 0; w < TapRows<ntaps>::WORDS; ++w) {
        srow1[0].rows[w] = half ? srow[1].rows[w] : srow[0].rows[w];
        srow1[0].swz[w] = half ? srow[1].swz[w] : srow[0].swz[w];
      }
      f32x4 acc[1];
      WSTAMP(4);
      job_weights(op, ct);
      for_kgroups(kgt, [&](auto kg) { wave_layer_kloop<ntaps, decltype(kg)::value, 1, PREC>(acc, net, op, srow1, ct, lane, bq, wv); });
      WSTAMP(0);
      wave_epilogue<PREC>(acc[0], net, op, half, ct, lane, rows);
      WSTAMP(1);
    }
    if (shared) pair_sync(flags, half, seq, lane);     // the layer is whole before either half reads it (or overwrites its source)
    else scs_sync<false>();                            // (this wavefront's own stores, then its own reads: LDS keeps their order)
    WSTAMP(2);
  }
}

// The ascending list of a position's legal actions: the mask in LDS, then its list (legal_list_of).  Returns their number.
__device__ __forceinline__ int legal_list_wave(const ScsRules& R, const ScsState& sc, uint32_t* smask, int* sidx, int lane) {
  scs_legal_mask_wave<MASK_WORDS, false>(R, sc, smask, lane);
  return legal_list_of([&](int w) { return w * 64 + lane < MASK_WORDS ? smask[w * 64 + lane] : 0u; }, sidx, lane);
}
// This wavefront's half (`half` = 0 leader, 1 helper) of turning the staged float32 planes into the input pieces (every
// row of the input region, its row of zeros included) ...
// (plain-bf16 mode: piece 0 is the planes rounded to nearest even, pieces 1 and 2 are stored as zeros -- the space is the
// logits', the value plane's and a hidden buffer's afterwards, and what their K groups' padding reads must be numbers)
template <int PREC = PREC_F32>
__device__ __forceinline__ void split_planes_half(float* __restrict__ net, const PersistArgs& q, const WaveNetArgs& wn, int lane,
                                                  int half) {
  const int hw = wn.rows, in_off = wn.in_off, in_cs = wn.in_cs;
  const float* const stage = net + q.stage_off;
  const int chunks = q.inp >> 3;
  for (int i = lane + 64 * half; i < (hw + 1) * chunks; i += 128) {
    const int r = i / chunks, c8 = i - r * chunks;
    u32x4 q0 = u32x4{0u, 0u, 0u, 0u}, q1 = q0, q2 = q0;
    if (r < hw) {
      f32x4 lo4 = *reinterpret_cast<const f32x4*>(stage + r * q.inp + c8 * 8);
      f32x4 hi4 = *reinterpret_cast<const f32x4*>(stage + r * q.inp + c8 * 8 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (c8 * 8 + j >= q.in_channels) lo4[j] = 0.f;
        if (c8 * 8 + 4 + j >= q.in_channels) hi4[j] = 0.f;
      }
      if constexpr (PREC == PREC_BF16) q0 = round8(lo4, hi4);
      else split8(lo4, hi4, q0, q1, q2);
    }
    float* d = net + in_off + r * in_cs + (c8 >> 2) * GROUP_FLOATS + (((c8 & 3) ^ ((r >> 2) & 3)) << 2);
    *reinterpret_cast<u32x4*>(d) = q0;
    *reinterpret_cast<u32x4*>(d + PIECE_FLOATS) = q1;
    *reinterpret_cast<u32x4*>(d + 2 * PIECE_FLOATS) = q2;
  }
}
// ... and of zeroing the staging space again (it lies over the trunk buffers: their rows of zeros, channels no layer writes)
__device__ __forceinline__ void zero_stage_half(float* __restrict__ net, const PersistArgs& q, int lane, int half) {
  float* const stage = net + q.stage_off;
  for (int i = (lane + 64 * half) * 4; i < q.stage_floats; i += 512) *reinterpret_cast<f32x4*>(stage + i) = f32x4{0.f, 0.f, 0.f, 0.f};
}

// the search of one game's move: the leader wavefront's body (returns when the move's simulations are used up)
template <bool HEX, int CH = MAXC_CHUNKS, int PREC = PREC_F32>
__device__ __forceinline__ void persist_leader(const SearchParams& p, const PersistArgs& q, const ScsRules& R, unsigned char* wb,
                                               int g, const int lane_in, int* flags, int* go) {
  int lane = lane_in;
  ScsState& real_l = *reinterpret_cast<ScsState*>(wb);
  ScsState& sc = *reinterpret_cast<ScsState*>(wb + PERSIST_STATE_BYTES);
  int* const sidx = reinterpret_cast<int*>(wb + 2 * PERSIST_STATE_BYTES + PERSIST_MASK_BYTES);
  float* const net = reinterpret_cast<float*>(wb + PERSIST_GAME_BYTES);
  int seq = 0, pass = 0;
  if (p.real[g].terminal) return;
  int sims_left = p.sims_left[g];
  if (sims_left <= 0) return;
  const int root = p.root[g];
  int base = p.node_count[g];
  int32_t* const path = p.path + (size_t)g * p.max_path;
  SNode* const nodes = arena(p, g);
  const int A = p.num_actions;
  {   // the real game and a clean network block
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&p.real[g]);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&real_l);
    for (int i = lane; i < (int)(sizeof(ScsState) / 4); i += 64) dst[i] = src[i];
    for (int i = lane * 4; i < q.net_floats; i += 256) *reinterpret_cast<f32x4*>(net + i) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int rec = q.rec_slot ? q.rec_slot[g] : -1;
  int rec_n = rec >= 0 ? q.rec_count[rec] : 0;
  const WaveNetArgs wna = wave_net_args(q.prog, lane);
  const int hw = wna.rows, pp = wna.pol_cs;
  scs_sync<false>();
  int n_sim = 0, n_exp = 0, n_hit = 0, n_miss = 0;      // (of this move: 32 bits are plenty, and half the registers)
  bool failed = false;
  const uint32_t tiles_magic = 0xFFFFFFFFu / (uint32_t)hw + 1u;       // ceil(2^32 / tiles) for scs_step_wave (exact for every action index of boards of <= 100 tiles: checked exhaustively on the host, tests/test_host_logic.py)
#ifdef NZ_PERSIST_STAMPS   // diagnostic build: where a game's time goes (nz_scs_search_persist_ticks)
  unsigned long long tk[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, ts = __builtin_amdgcn_s_memtime();
  const unsigned long long t_begin = ts;
#define PSTAMP(slot) { const unsigned long long now = __builtin_amdgcn_s_memtime(); tk[slot] += now - ts; ts = now; }
#else
#define PSTAMP(slot)
#endif

  while (sims_left > 0) {
    // (an opaque lane id per simulation: what is derived from it is a few cheap instructions, and carried around the
    // whole loop instead it is a dozen registers spilled to scratch and reloaded in the middle of the tree phase)
    lane = lane_in;
    asm volatile("" : "+v"(lane));
    {   // scratch_game = game.shallow_clone()
      const uint32_t* src = reinterpret_cast<const uint32_t*>(&real_l);
      uint32_t* dst = reinterpret_cast<uint32_t*>(&sc);
      for (int i = lane; i < (int)(sizeof(ScsState) / 4); i += 64) dst[i] = src[i];
      scs_sync<false>();
    }
    PSTAMP(0);                                  // clone
    int node = root, plen = 1;
    int my_path = root;                         // lane i holds path[i] (levels past 63 go to memory)
    bool bad = false;
    Level par = level_of(nodes[root]);
    // A level's children (its first 64) and its two table entries are fetched BEFORE the rule step that leads to it:
    // the round trip to L2 runs under the step's serial code instead of after it.
    SNode cnext;
    double sq = 0.0, cb = 0.0;
    auto fetch_level = [&]() {
      if (lane < par.n_children) cnext = nodes[par.child_base + lane];
      if (par.visit < p.tab_len) { sq = p.sqrt_tab[par.visit]; cb = p.bias_tab[par.visit]; }
    };
    fetch_level();
    while (par.n_children > 0) {
      if (par.visit >= p.tab_len || plen >= p.max_path) { bad = true; break; }
      const int key = select_level(p, nodes, par, sq, cb, lane, [&](int) { return cnext; }, node);
      if (par.n_children > 0) fetch_level();
      if (plen < 64) { if (lane == plen) my_path = node; }
      else if (lane == 0) path[plen] = node;
      scs_step_wave<false>(R, sc, key >> 8, lane, tiles_magic);
      ++plen;
    }
    if (bad) {
      if (lane == 0) atomicOr(p.error_flag, 2);
      failed = true;
      break;
    }
    scs_sync<false>();
    PSTAMP(1);                                  // descent: scores, argmax, rule steps
    const int to_play = sc.player, term = sc.terminal;
    double v;
    if (term) {                                 // Explorer.py:140-142: the stored terminal value, no network
      if (lane == 0) {
        nodes[node].to_play = (int8_t)to_play;
        nodes[node].terminal = 1;
      }
      v = (double)sc.terminal_value;
    } else {
      if (lane == 0) nodes[node].to_play = (int8_t)to_play;
      // The helper wavefront starts NOW on the leaf's legal mask and list (it is needed only at the expansion), while this
      // one looks the leaf up in the cache and stages its planes; they meet before the planes are split.
      ++pass;
      if (lane == 0) flags[7] = base;             // (what the helper's own overflow check needs)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");   // (the helper reads LDS only: no wait for the stores to the tree)
      if (lane == 0) __hip_atomic_store(go, pass, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#ifdef NZ_PERSIST_STAMP_GO    // diagnostic of a diagnostic: the leaf's bookkeeping up to the helper's wake-up, reported in the "slowest" slot
      PSTAMP(9);
#endif
      float* const pol = net + wna.pol_off;
      float sum = 1.0f, value = 0.f;
      // The inference cache (Explorer.py:146-155): the table is shared by every game of the engine and, on this route, read
      // and written while the kernel runs -- by games on all eight XCDs, so every access is an agent-scope atomic (past this
      // CU's L1 and this XCD's L2) and there are no fences (agent-scope fences write back / invalidate whole caches: 817
      // games/s with them against 970 without a cache).  Entries validate themselves: next to the state's 128-bit key an
      // entry holds a 64-bit check word over (key, probabilities, value); a reader takes everything in ONE round of loads
      // and accepts it only if the key is its leaf's and the check word fits what it read -- an entry caught half
      // written, or written by two games at once, fails and counts as a miss.  Writers just store (newest wins,
      // KeylessCache.py:60-75).  A hit is the evaluation the network made for the same state: the search cannot tell.
      uint64_t key_hi = 0, key_lo = 0;
      size_t entry = 0;
      bool hit = false;
      if (p.c_bits > 0) {
        entry = (size_t)uniform64(leaf_cache_key(p, g, sc, lane, key_hi, key_lo));
        key_hi = uniform64(key_hi); key_lo = uniform64(key_lo);         // (the same on every lane: scalar registers)
        unsigned long long* const id = reinterpret_cast<unsigned long long*>(p.c_id + 2 * entry);
        const unsigned long long id0 = __hip_atomic_load(id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long id1 = __hip_atomic_load(id + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long chk = __hip_atomic_load(reinterpret_cast<unsigned long long*>(p.c_check + entry), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float cval = __hip_atomic_load(p.c_value + entry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint64_t acc = 0;
        {   // (all of a block's loads in flight together: one round trip to memory, not one per probability -- which is
            // why this walk over the actions is not for_each_action's: that one hands out an entry at a time)
          constexpr int PER = 12;
          int cell = lane % hw, plane = lane / hw;
          const int dcell = 64 % hw, dplane = 64 / hw;
          for (int i0 = 0; i0 < A; i0 += 64 * PER) {
            float r[PER];
#pragma unroll
            for (int j = 0; j < PER; ++j) {
              const int i = i0 + j * 64 + lane;
              r[j] = i < A ? __hip_atomic_load(p.c_probs + entry * A + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
            }
#pragma unroll
            for (int j = 0; j < PER; ++j) {
              const int i = i0 + j * 64 + lane;
              if (i < A) {
                pol[cell * pp + plane] = r[j];
                acc += check_term(i, r[j]);
              }
              cell += dcell; plane += dplane;
              if (cell >= hw) { cell -= hw; ++plane; }
            }
          }
        }
        hit = id0 == key_hi && id1 == key_lo && cache_check_word(acc, cval, key_hi, key_lo) == chk;     // (uniform)
        if (hit) { value = cval; ++n_hit; } else ++n_miss;
        scs_sync<false>();
      }
      uint64_t dig_hi = 0, dig_lo = 0;
      if (hit && rec >= 0) {                    // (the test hook records every evaluation the search consumed: the planes' digest)
        float* const stage = net + q.stage_off;
        scs_state_image_wave<true, true>(R, sc, stage, q.inp >> 4, lane);
        scs_sync<false>();
        image_hash_wave(stage, q.inp, q.in_channels, hw, lane, dig_hi, dig_lo);
        scs_sync<false>();
        for (int i = lane * 4; i < q.stage_floats; i += 256) *reinterpret_cast<f32x4*>(stage + i) = f32x4{0.f, 0.f, 0.f, 0.f};
        scs_sync<false>();
      }
      if (!hit) {
        // the leaf's planes (generate_network_input, SCS_Game.py:1507) as float32 rows over the trunk buffers' space
        float* const stage = net + q.stage_off;
        scs_state_image_wave<true, true>(R, sc, stage, q.inp >> 4, lane);
        scs_sync<false>();
        if (rec >= 0) image_hash_wave(stage, q.inp, q.in_channels, hw, lane, dig_hi, dig_lo);
      }
      PSTAMP(2);                                // cache lookup + planes (the helper: legal mask + list)
      if (lane == 0) flags[5] = hit ? 0 : 1;      // what the helper does after the meeting: nothing more / its half of the pass
      pair_sync(flags, 0, seq, lane);
      const int k = flags[6];                     // the helper's count of legal actions (the list is in sidx)
      {
        const bool overflow = k > p.maxc;
        if (overflow || base + k > p.half_cap) {  // (the helper makes the same check and stops here too)
          if (lane == 0) atomicOr(p.error_flag, overflow ? 16 : 1);
          failed = true;
          break;
        }
      }
      if (!hit) {
      split_planes_half<PREC>(net, q, wna, lane, 0);
      scs_sync<false>();
      pair_sync(flags, 0, seq, lane);             // (both halves of the pieces are made: the staging space can go)
      zero_stage_half(net, q, lane, 0);
      scs_sync<false>();
      pair_sync(flags, 0, seq, lane);
      PSTAMP(3);                                // split, staging cleared (halves)
#ifdef NZ_PERSIST_STAMPS
      wave_network<HEX, PREC>(wna, net, lane, 0, flags, seq, tk + 10);
#else
      wave_network<HEX, PREC>(wna, net, lane, 0, flags, seq);
#endif
      PSTAMP(4);                                // network

      // softmax over ALL logits (Explorer.py:158-160) and value = tanh(mean of the value plane) (blocks.py:82-84)
      float mx = -INFINITY;
      for_each_action(A, hw, lane, 64, [&](int, int cell, int plane) { mx = fmaxf(mx, pol[cell * pp + plane]); });
      for (int w = 32; w; w >>= 1) mx = fmaxf(mx, __shfl_xor(mx, w, 64));
      // the sum in the order fused16_net_kernel gives a workgroup's only position (softmax_ways), all partial sums on this
      // wavefront, so that a game plays the same moves on either route
      constexpr int WAYS = softmax_ways(1);
      static_assert(WAYS == softmax_ways(4), "the wave-by-wave route's workgroups hold up to four positions");
      float part[WAYS] = {};
      for_each_action_blocked<WAYS>(A, hw, lane, 64, [&](int, int cell, int plane, int sub) {
        const float e = expf(pol[cell * pp + plane] - mx);
        pol[cell * pp + plane] = e;
        part[sub] += e;
      });
      sum = 0.f;
#pragma unroll
      for (int sub = 0; sub < WAYS; ++sub) sum += wave_sum(part[sub]);
      pair_sync(flags, 0, seq, lane);             // (the helper's value head is done)
      value = value_of_plane(lane < hw ? net[wna.val_off + lane * wna.val_cs] : 0.f, hw);       // (hw <= 64: a cell per lane)
      scs_sync<false>();
      PSTAMP(5);                                // softmax + value
      if (p.c_bits > 0) {
        // KeylessCache.put (KeylessCache.py:60-75): the newest evaluation takes the entry; stores only, nothing to wait for
        unsigned long long* const id = reinterpret_cast<unsigned long long*>(p.c_id + 2 * entry);
        uint64_t acc = 0;
        for_each_action(A, hw, lane, 64, [&](int i, int cell, int plane) {
          const float pr = pol[cell * pp + plane] / sum;
          __hip_atomic_store(p.c_probs + entry * A + i, pr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          acc += check_term(i, pr);
        });
        const unsigned long long chk = cache_check_word(acc, value, key_hi, key_lo);
        if (lane == 0) {
          __hip_atomic_store(p.c_value + entry, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(id, (unsigned long long)key_hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(id + 1, (unsigned long long)key_lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(reinterpret_cast<unsigned long long*>(p.c_check + entry), chk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      }   // (!hit)
      v = (double)value;
      if (rec >= 0) {
        if (rec_n < q.rec_cap) {
          const size_t at = (size_t)rec * q.rec_cap + rec_n;
          for_each_action(A, hw, lane, 64, [&](int i, int cell, int plane) { q.rec_probs[at * A + i] = pol[cell * pp + plane] / sum; });
          if (lane == 0) { q.rec_value[at] = value; q.rec_digest[2 * at] = dig_hi; q.rec_digest[2 * at + 1] = dig_lo; }
        }
        ++rec_n;
      }
      // expansion: the j-th legal action and its probability for expand_children
      int my_idx[CH];                        // (CH = 1: this game has at most 64 legal actions in a position)
      float my_val[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int j = c * 64 + lane;
        my_idx[c] = j < k ? sidx[j] : 0x7fffffff;
        float pr = 0.0f;
        if (j < k) {
          const int plane = my_idx[c] / hw, cell = my_idx[c] - plane * hw;
          pr = pol[cell * pp + plane] / sum;
        }
        my_val[c] = pr;
      }
      expand_children<CH>(p, nodes, node, base, k, lane, my_idx, my_val);
      base += k;
      ++n_exp;
      PSTAMP(6);                                // expansion
    }
    // backup: levels 0..63 from the lanes' registers, the rest from memory
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (lane < plen && lane < 64) backup_node(nodes[my_path], v);
    backup_tail(nodes, path, 64, plen, lane, v);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    --sims_left;
    ++n_sim;
    PSTAMP(7);                                  // backup
  }
#ifdef NZ_PERSIST_STAMPS
  if (lane == 0) {
    tk[8] = __builtin_amdgcn_s_memtime() - t_begin;        // the game's whole move
    for (int i = 0; i < 6; ++i) atomicAdd((unsigned long long*)&p.counters[2 + i], tk[i]);
    for (int i = 6; i < 9; ++i) atomicAdd((unsigned long long*)&p.counters[5 + i], tk[i]);
#ifdef NZ_PERSIST_STAMP_GO
    atomicAdd((unsigned long long*)&p.counters[14], tk[9]);
#else
    atomicMax((unsigned long long*)&p.counters[14], tk[8]);  // the slowest (game, move) of the round
#endif
    // inside the network (the leader's half): K loops, epilogues, waiting for the helper -- in the cache counters' words
    // (a diagnostic build runs without the cache)
    for (int i = 0; i < 3; ++i) atomicAdd((unsigned long long*)&p.counters[8 + i], tk[10 + i]);
  }
#endif
  if (lane == 0) {
    p.sims_left[g] = failed ? sims_left : 0;
    p.pending[g] = -1;
    p.node_count[g] = base;
    if (rec >= 0) q.rec_count[rec] = rec_n;
    if (n_sim) atomicAdd((unsigned long long*)&p.counters[0], (unsigned long long)n_sim);
    if (n_exp) atomicAdd((unsigned long long*)&p.counters[1], (unsigned long long)n_exp);
    if (n_hit) atomicAdd((unsigned long long*)&p.counters[8], (unsigned long long)n_hit);
    if (n_miss) atomicAdd((unsigned long long*)&p.counters[9], (unsigned long long)n_miss);
  }
}

template <bool HEX, int CH = MAXC_CHUNKS, int PREC = PREC_F32>
__global__ __launch_bounds__(PERSIST_THREADS) void persist_kernel(SearchParams p, PersistArgs q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // wavefronts 0..3 lead games 0..3; wavefront 4 + i helps game (i + 3) & 3, so that every SIMD hosts one leader and
  // one helper of ANOTHER game (a helper sleeps through its game's tree phases)
  const bool leader = wave < PERSIST_GAMES;
  const int slot = leader ? wave : ((wave - PERSIST_GAMES + 3) & (PERSIST_GAMES - 1));
  const int n_rules = q.rules_per_game ? PERSIST_GAMES : 1;       // descriptions in LDS: one, or one per game slot (its own map)
  const ScsRules& R = *reinterpret_cast<const ScsRules*>(smem + (size_t)(q.rules_per_game ? slot : 0) * PERSIST_RULES_BYTES);
  {   // rules -> LDS, once per workgroup, and the games' flag words; the only workgroup barrier of the kernel
    static_assert(sizeof(ScsRules) % 4 == 0 && sizeof(ScsState) % 4 == 0, "copied as dwords");
    for (int r = 0; r < n_rules; ++r) {
      const int gr = blockIdx.x * PERSIST_GAMES + r;
      if (gr >= p.n_games) break;
      const uint32_t* src = reinterpret_cast<const uint32_t*>(&rules_of(p, gr));
      uint32_t* dst = reinterpret_cast<uint32_t*>(smem + (size_t)r * PERSIST_RULES_BYTES);
      for (int i = threadIdx.x; i < (int)(sizeof(ScsRules) / 4); i += PERSIST_THREADS) dst[i] = src[i];
    }
    if (threadIdx.x < PERSIST_GAMES * 8)
      reinterpret_cast<int*>(smem + (size_t)n_rules * PERSIST_RULES_BYTES + (size_t)(threadIdx.x >> 3) * q.wave_bytes + PERSIST_GAME_BYTES - PERSIST_FLAG_BYTES)[threadIdx.x & 7] = 0;
  }
  __syncthreads();
  unsigned char* const wb = smem + (size_t)n_rules * PERSIST_RULES_BYTES + (size_t)slot * q.wave_bytes;
  int* const flags = reinterpret_cast<int*>(wb + PERSIST_GAME_BYTES - PERSIST_FLAG_BYTES);
  int* const go = flags + 4;
  const int g = blockIdx.x * PERSIST_GAMES + slot;
  if (leader) {
    if (g < p.n_games) persist_leader<HEX, CH, PREC>(p, q, R, wb, g, lane, flags, go);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_store(go, PERSIST_EXIT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return;
  }
  // helper: half of every layer of every network pass of its game, asleep in between
  float* const net = reinterpret_cast<float*>(wb + PERSIST_GAME_BYTES);
  const WaveNetArgs wna = wave_net_args(q.prog, lane);
  const ScsState& sc = *reinterpret_cast<const ScsState*>(wb + PERSIST_STATE_BYTES);
  uint32_t* const smask = reinterpret_cast<uint32_t*>(wb + 2 * PERSIST_STATE_BYTES);
  int* const sidx = reinterpret_cast<int*>(wb + 2 * PERSIST_STATE_BYTES + PERSIST_MASK_BYTES);
  int seq = 0, pass = 0;
  for (;;) {
    int gv;
    while ((gv = __hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == pass) __builtin_amdgcn_s_sleep(2);
    if (gv == PERSIST_EXIT) break;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    pass = gv;
    // a leaf that needs an evaluation: its legal mask and list (the leader meanwhile looks it up in the cache and stages
    // its planes), then -- unless the cache had it -- half of the split into pieces and half of every layer
    const int k = legal_list_wave(R, sc, smask, sidx, lane);
    if (lane == 0) flags[6] = k;
    pair_sync(flags, 1, seq, lane);
    const int job = flags[5], base = flags[7];
    if (job == 0 || k > p.maxc || base + k > p.half_cap) continue;     // (a hit, or the leader is raising the overflow flag)
    split_planes_half<PREC>(net, q, wna, lane, 1);
    scs_sync<false>();
    pair_sync(flags, 1, seq, lane);
    zero_stage_half(net, q, lane, 1);
    scs_sync<false>();
    pair_sync(flags, 1, seq, lane);
    wave_network<HEX, PREC>(wna, net, lane, 1, flags, seq);
    pair_sync(flags, 1, seq, lane);               // (the value plane is whole; the leader has done its softmax meanwhile)
  }
}

// Diagnostic: the network part of persist_kernel alone -- every game slot of every workgroup runs `iters` passes on an
// all-zero input (leader + helper exactly as in the search), out[block * PERSIST_GAMES + slot] = shader ticks per pass.
template <bool HEX, int PREC = PREC_F32>
__global__ __launch_bounds__(PERSIST_THREADS) void netbench_kernel(PersistArgs q, int iters, unsigned long long* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool leader = wave < PERSIST_GAMES;
  const int slot = leader ? wave : ((wave - PERSIST_GAMES + 3) & (PERSIST_GAMES - 1));
  if (threadIdx.x < PERSIST_GAMES * 8)
    reinterpret_cast<int*>(smem + PERSIST_RULES_BYTES + (size_t)(threadIdx.x >> 3) * q.wave_bytes + PERSIST_GAME_BYTES - PERSIST_FLAG_BYTES)[threadIdx.x & 7] = 0;
  __syncthreads();
  unsigned char* const wb = smem + PERSIST_RULES_BYTES + (size_t)slot * q.wave_bytes;
  int* const flags = reinterpret_cast<int*>(wb + PERSIST_GAME_BYTES - PERSIST_FLAG_BYTES);
  float* const net = reinterpret_cast<float*>(wb + PERSIST_GAME_BYTES);
  const WaveNetArgs wna = wave_net_args(q.prog, lane);
  if (leader)
    for (int i = lane * 4; i < q.net_floats; i += 256) *reinterpret_cast<f32x4*>(net + i) = f32x4{0.f, 0.f, 0.f, 0.f};
  int seq = 0;
  pair_sync(flags, leader ? 0 : 1, seq, lane);
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  unsigned long long* tkn = nullptr;
#ifdef NZ_PERSIST_STAMPS
  unsigned long long phase_ticks[5] = {0, 0, 0, 0, 0};   // K loops, epilogues, meetings, first operands (HEADSTAMP), layer headers
  tkn = phase_ticks;
#endif
  const int active = (iters >> 16) & 0xff ? (iters >> 16) & 0xff : PERSIST_GAMES, n_it = iters & 0xffff;
  if (slot < active)
    for (int it = 0; it < n_it; ++it) {
      wave_network<HEX, PREC>(wna, net, lane, leader ? 0 : 1, flags, seq, tkn);
      pair_sync(flags, leader ? 0 : 1, seq, lane);
    }
  unsigned long long rep = __builtin_amdgcn_s_memtime() - t0;
  bool reports = leader;
#ifdef NZ_PERSIST_STAMPS    // diagnostic build: iters bits 24.. = 1 + the phase whose ticks are reported instead of the pass
  const int phase = (iters >> 24) - 1;
  for (int k = 0; k < 5; ++k) if (phase == k) rep = tkn[k];
  if (phase >= 8 && phase < 13) {              // phases 8..12: the HELPER's
    rep = tkn[phase - 8];
    reports = !leader;
  }
#endif
  if (reports && lane == 0) out[blockIdx.x * PERSIST_GAMES + slot] = rep / (unsigned long long)n_it;
}

__global__ void search_status_kernel(SearchParams p, int32_t* out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.n_games) return;
  const ScsState& s = p.real[g];
  int32_t* o = out + g * 7;
  o[0] = s.player; o[1] = s.sub_phase; o[2] = s.stage; o[3] = s.turn; o[4] = s.terminal; o[5] = s.terminal_value;
  o[6] = s.length;
}

// select_action, records, step and re-rooting (Explorer.py:70-97,183-199; Gamer.py:71-79)
// `forced` (may be null): per game an action to play instead of the search's own choice, -1 = own choice -- the
// opponent's move in MctsAgent.update_subtree (Testing/Agents/Generic/MctsAgent.py:35-39)
__global__ void end_move_kernel(SearchParams p, const double* __restrict__ uniforms, const int32_t* __restrict__ forced) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.n_games) return;
  ScsState& real = p.real[g];
  if (real.terminal) return;
  const ScsRules& R = rules_of(p, g);
  SNode* nodes = arena(p, g);
  const SNode root = nodes[p.root[g]];
  const int k = root.n_children, move = real.length;
  if (k == 0 || p.sims_left[g] != 0 || p.pending[g] >= 0 || move >= p.max_moves) {
    // a searched root without a child: a live position without a legal action ("Dead ends").  The move's
    // simulations all evaluated the root; the reference raises in max_action here.  The first game to say so is named.
    const bool dead_end = k == 0 && p.sims_left[g] == 0 && p.pending[g] < 0 && move < p.max_moves;
    atomicOr(p.error_flag, move >= p.max_moves ? 32 : dead_end ? 128 : 4);
    if (dead_end && atomicCAS(&p.error_flag[1], -1, g) == -1) p.error_flag[2] = move;
    return;
  }
  const size_t gm = (size_t)g * p.max_moves + move;
  const int MAXC = p.maxc;
  int best = 0;
  for (int j = 0; j < k; ++j) {
    const SNode& c = nodes[root.child_base + j];
    p.rec_child_action[gm * MAXC + j] = c.action;
    p.rec_child_visit[gm * MAXC + j] = c.visit;
    p.rec_child_prior[gm * MAXC + j] = c.prior;
    p.rec_child_value_sum[gm * MAXC + j] = c.value_sum;
    if (c.visit > nodes[root.child_base + best].visit) best = j;      // max_action: first maximum
  }
  p.rec_tree_size[gm] = root.visit;
  p.rec_children[gm] = k;
  p.rec_bias[gm] = root.visit < p.tab_len ? p.bias_tab[root.visit] : 0.0;
  p.rec_root_value_sum[gm] = root.value_sum;

  int mode = 0;
  double u3 = 0.0;
  const int forced_action = forced ? forced[g] : -1;
  if (forced_action >= 0) {
    mode = 3;
  } else if (p.training) {
    const double u1 = uniforms[g * 3], u2 = uniforms[g * 3 + 1];
    u3 = uniforms[g * 3 + 2];
    if (move < p.softmax_moves) mode = 1;
    else if (u1 < p.eps_softmax) mode = 1;
    else if (u2 < p.eps_random) mode = 2;
  }
  int chosen_child = best;
  if (mode == 1) {                         // softmax_action (Explorer.py:187-199)
    double e[MAXC_LIMIT];
    int mx = 0;
    for (int j = 0; j < k; ++j) mx = max(mx, nodes[root.child_base + j].visit);
    for (int j = 0; j < k; ++j) e[j] = exp((double)(nodes[root.child_base + j].visit - mx));
    const double s = np_sum_f64(e, k);
    for (int j = 0; j < k; ++j) e[j] = e[j] / s;
    const double s2 = np_sum_f64(e, k);
    double run = 0.0, last;
    for (int j = 0; j < k; ++j) { e[j] = e[j] / s2; }
    for (int j = 0; j < k; ++j) { run = j == 0 ? e[0] : run + e[j]; e[j] = run; }
    last = e[k - 1];
    chosen_child = k - 1;
    for (int j = 0; j < k; ++j) if (e[j] / last > u3) { chosen_child = j; break; }
  } else if (mode == 2) {                  // uniform over the legal actions (Explorer.py:86-89)
    // p = mask / n_valid over all actions; cdf = cumsum(p) / cdf[-1]; searchsorted(u, 'right').
    // The root's children are exactly the legal actions, in ascending order.
    const double pv = 1.0 / (double)k;     // 1 / np.sum(mask): int8 sum -> exact integer
    double run = 0.0;
    double cdf[MAXC_LIMIT];
    for (int j = 0; j < k; ++j) { run = j == 0 ? pv : run + pv; cdf[j] = run; }
    chosen_child = k - 1;
    for (int j = 0; j < k; ++j) if (cdf[j] / cdf[k - 1] > u3) { chosen_child = j; break; }
  }
  if (mode == 3) {
    chosen_child = -1;
    for (int j = 0; j < k; ++j)
      if (nodes[root.child_base + j].action == forced_action) chosen_child = j;
    if (chosen_child < 0) {                  // not a legal move of this position
      atomicOr(p.error_flag, 8);
      return;
    }
  }
  const int action = nodes[root.child_base + chosen_child].action;
  p.rec_action[gm] = action;
  Scs(R, real).step(action);
  p.root[g] = root.child_base + chosen_child;
}

// Re-rooting (Gamer.py:78-79) with the dead part of the tree dropped: the subtree of the new root is copied
// breadth-first into the other half of the game's arena (a node's children stay one contiguous block in the same
// order, so nothing observable changes), the old half is free for the move after next.  One wavefront per game:
// lane i takes the i-th node of the current BFS window and copies its block of children.
__global__ __launch_bounds__(64) void compact_kernel(SearchParams p) {
  const int g = blockIdx.x;
  const int lane = lane_id();
  if (p.real[g].terminal) return;
  const SNode* src = arena(p, g);
  SNode* dst = p.nodes + (size_t)g * p.cap + (size_t)(p.half[g] ^ 1) * p.half_cap;
  if (lane == 0) dst[0] = src[p.root[g]];
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  int count = 1, head = 0;
  while (head < count) {
    const int window = count - head < 64 ? count - head : 64;     // nodes whose children are copied this round
    const int i = head + lane;
    int k = 0, cb = 0;
    if (lane < window) { k = dst[i].n_children; cb = dst[i].child_base; }
    int inc = k;
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    const int total = __shfl(inc, 63, 64);
    // (cannot trigger: the subtree copied here is part of a tree that fits the other half, and the halves are the same
    // size -- the searches' own checks report a full arena.  Kept as the bound on the stores below; no test reaches it.)
    if (count + total > p.half_cap) {                  // uniform
      if (lane == 0) atomicOr(p.error_flag, 1);
      return;
    }
    if (k > 0) {
      const int at = count + inc - k;
      for (int j = 0; j < k; ++j) dst[at + j] = src[cb + j];
      dst[i].child_base = at;
    }
    count += total;
    head += window;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  if (lane == 0) {
    p.half[g] ^= 1;
    p.root[g] = 0;
    p.node_count[g] = count;
  }
}

// the persistent kernel for a network (square / hexagonal taps), wavefronts per game and the game's children bound
// (at most 64 legal actions per position: the expansion handles one chunk of children instead of four)
typedef void (*persist_fn_t)(SearchParams, PersistArgs);
persist_fn_t persist_pick(bool hex, bool one_chunk, int precision) {
  if (precision == NZ_PREC_BF16) {
    if (hex) return one_chunk ? persist_kernel<true, 1, PREC_BF16> : persist_kernel<true, MAXC_CHUNKS, PREC_BF16>;
    return one_chunk ? persist_kernel<false, 1, PREC_BF16> : persist_kernel<false, MAXC_CHUNKS, PREC_BF16>;
  }
  if (hex) return one_chunk ? persist_kernel<true, 1> : persist_kernel<true, MAXC_CHUNKS>;
  return one_chunk ? persist_kernel<false, 1> : persist_kernel<false, MAXC_CHUNKS>;
}


// ---- who owns the handle's memory --------------------------------------------------------------------------------------
// One struct of owners (hip_own.hpp) per lifecycle: ensure() is all or nothing -- a group that could not be made whole is
// emptied, so the next call tries again and nothing ever runs on half of one -- and bind() is the only code that writes
// the group's pointers into the kernels' argument structs (null after a reset).
template <typename Group>
bool whole(Group* g, bool ok) {
  if (!ok) *g = Group{};
  return ok;
}

struct CreateBufs {               // nz_scs_search_create, for the handle's life
  DevBuf<ScsRules> rules;         // the description (one row)
  DevBuf<ScsState> real, scratch;
  DevBuf<SNode> nodes;
  DevBuf<int32_t> node_count, root, sims_left, pending, path, path_len, error_flag;
  DevBuf<int32_t> leaf_count;     // 6 ints: two (leaf, active, cache hit) triples
  DevBuf<int8_t> half; DevBuf<uint32_t> leaf_mask; DevBuf<int64_t> counters;
  DevBuf<double> bias_tab, sqrt_tab;
  DevBuf<int32_t> rec_action, rec_tree_size, rec_children, rec_child_action, rec_child_visit;
  DevBuf<double> rec_bias, rec_root_value_sum, rec_child_prior, rec_child_value_sum;
  // makes the arrays and hands them to `p` (p.rules: GameRows::bind; the counter triple: rest_counters)
  bool ensure(SearchParams& p) {
    const size_t G = p.n_games, GM = G * p.max_moves, GMC = GM * p.maxc, tab = p.tab_len;
#define MADE(f, n) (f.ensure(n) && (p.f = f.get()))
    return whole(this, rules.ensure(1) && leaf_count.ensure(6) && MADE(real, G) && MADE(scratch, G) && MADE(nodes, G * (size_t)p.cap) &&
                           MADE(half, G) && MADE(node_count, G) && MADE(root, G) && MADE(sims_left, G) && MADE(pending, G) &&
                           MADE(path, G * (size_t)p.max_path) && MADE(path_len, G) && MADE(leaf_mask, G * MASK_WORDS) && MADE(error_flag, 3) &&
                           MADE(counters, 16) && MADE(bias_tab, tab) && MADE(sqrt_tab, tab) && MADE(rec_action, GM) && MADE(rec_tree_size, GM) &&
                           MADE(rec_children, GM) && MADE(rec_bias, GM) && MADE(rec_root_value_sum, GM) && MADE(rec_child_action, GMC) &&
                           MADE(rec_child_visit, GMC) && MADE(rec_child_prior, GMC) && MADE(rec_child_value_sum, GMC));
#undef MADE
  }
};

struct PlayBufs {                 // the library's move loop: leaf batch, evaluations, one move's host-drawn randomness
  DevBuf<float> probs, value;     // evaluations: the network's in slots [0, G), cache hits in [G, 2 G) / [2 G, 3 G) by wave parity
  DevBuf<int32_t> leaf_game, nchild, status;
  DevBuf<uint64_t> leaf_key;
  DevBuf<double> noise, uniforms;
  PinnedBuf<int32_t> active;      // pinned host word + event: the early-finish poll of the wave-by-wave route
  Event ev_poll;
  bool ensure(size_t G, size_t A, size_t maxc) {
    return whole(this, probs.ensure(3 * G * A) && value.ensure(3 * G) && leaf_game.ensure(G) && leaf_key.ensure(2 * G) &&
                           nchild.ensure(G) && status.ensure(G * 7) && noise.ensure(G * maxc) && uniforms.ensure(G * 3) &&
                           active.ensure(1) && ev_poll.create(hipEventDisableTiming));
  }
  void bind(SearchParams& p) const { p.leaf_key = leaf_key.get(); p.eval_probs = probs.get(); p.eval_value = value.get(); }
};

struct RoundBufs {                // nz_scs_search_play_round: the round's store (grown, never shrunk), one move's slot bookkeeping
  DevBuf<int32_t> action, tree_size, children, child_action, child_visit, status, to_record, restart;
  DevBuf<double> bias, root_value_sum, child_prior, child_value_sum;
  int64_t games = 0;              // games the store holds
  bool ensure(int64_t n, size_t G, const SearchParams& p) {
    if (n <= games) return true;
    *this = RoundBufs{};          // every array grows with n: free them all before the first is made anew
    const size_t NM = (size_t)n * p.max_moves, NMC = NM * p.maxc;
    const bool ok = action.ensure(NM) && tree_size.ensure(NM) && children.ensure(NM) && bias.ensure(NM) && root_value_sum.ensure(NM) &&
                    child_action.ensure(NMC) && child_visit.ensure(NMC) && child_prior.ensure(NMC) && child_value_sum.ensure(NMC) &&
                    status.ensure((size_t)n * 2) && to_record.ensure(G) && restart.ensure(G);
    games = ok ? n : 0;
    return whole(this, ok);
  }
  void bind(RoundStore& r) const {
    r.action = action.get(); r.tree_size = tree_size.get(); r.children = children.get(); r.child_action = child_action.get();
    r.child_visit = child_visit.get(); r.status = status.get(); r.bias = bias.get(); r.root_value_sum = root_value_sum.get();
    r.child_prior = child_prior.get(); r.child_value_sum = child_value_sum.get();
  }
};

struct CacheBufs {                // nz_scs_search_cache: the inference cache's table
  DevBuf<uint64_t> id, check;
  DevBuf<float> probs, value;
  DevBuf<int32_t> writer;
  bool ensure(size_t n, size_t A) {
    return whole(this, id.ensure(n * 2) && probs.ensure(n * A) && value.ensure(n) && writer.ensure(n) && check.ensure(n));
  }
  void bind(SearchParams& p) const {
    p.c_id = id.get(); p.c_probs = probs.get(); p.c_value = value.get(); p.c_writer = writer.get(); p.c_check = check.get();
  }
};

struct RecordBufs {               // nz_scs_search_record: leaf evaluations of chosen games
  DevBuf<int32_t> slot, count;
  DevBuf<uint64_t> digest;
  DevBuf<float> probs, value;
  bool ensure(size_t G, size_t n, size_t capacity, size_t A) {
    const size_t N = n * capacity;
    return whole(this, slot.ensure(G) && count.ensure(n) && digest.ensure(N * 2) && probs.ensure(N * A) && value.ensure(N));
  }
  void bind(PersistArgs& q) const {
    q.rec_slot = slot.get(); q.rec_count = count.get(); q.rec_digest = digest.get(); q.rec_probs = probs.get(); q.rec_value = value.get();
  }
};

struct GameRows {                 // per-game maps (nz_scs_search_set_games / _draw_games); grown, never shrunk
  DevBuf<ScsRules> rules;         // [rows]
  DevBuf<uint64_t> key;           // [rows][2] map digests (the inference cache's key)
  DevBuf<int32_t> row;            // [n_games] the row each slot's game reads
  bool ensure(size_t n, size_t G) {
    if (n > rules.size()) { rules.reset(); key.reset(); }     // both grow: free both before either is made anew
    return whole(this, rules.ensure(n) && key.ensure(n * 2) && row.ensure(G));
  }
  // the plays read the per-game rows and digests, or the description's one map
  void bind(SearchParams& p, const ScsRules* base, bool per_game) const {
    p.rules = per_game ? rules.get() : base;
    p.rules_row = per_game ? row.get() : nullptr;
    p.rules_key = per_game ? key.get() : nullptr;
  }
};

struct DrawBufs {                 // nz_scs_search_draw_games: the last draw's per-game buffers (grown, never shrunk)
  DevBuf<uint32_t> seeds, keys;
  DevBuf<float> terrain;
  DevBuf<int32_t> vp, pos, err;
  bool ensure(size_t n, size_t tiles, size_t n_vp) {
    if (n > seeds.size()) *this = DrawBufs{};                 // all grow: free them all before the first is made anew
    return whole(this, seeds.ensure(n) && keys.ensure(n * 624) && terrain.ensure(n * tiles * 3) && vp.ensure(n * n_vp * 2) &&
                           pos.ensure(n) && err.ensure(n));
  }
};

struct MatchBufs {                // nz_scs_match_play, kept on agent 1's handle
  // the forced actions of both engines' end_move [2][G], the match record [G][max_moves], live matches and both engines' flags [3]
  DevBuf<int32_t> forced, actions, state;
  DevBuf<int64_t> tally;          // [8]
  PinnedBuf<int32_t> pinned;      // the (live, flags) read-back
  Stream stream;                  // the opponent's search
  Event ev_fork, ev_join;
  bool ensure(size_t G, size_t max_moves) {
    return whole(this, forced.ensure(2 * G) && actions.ensure(G * max_moves) && state.ensure(3) && tally.ensure(8) && pinned.ensure(3) &&
                           stream.create(hipStreamNonBlocking) && ev_fork.create(hipEventDisableTiming) &&
                           ev_join.create(hipEventDisableTiming));
  }
};

struct AgentSideBufs {            // one scripted side of nz_scs_agent_match_play
  DevBuf<uint32_t> seeds, mt_keys;               // random agent: the matches' seeds and MT19937 states
  DevBuf<int32_t> mt_pos, count;
  DevBuf<float> probs, value;                    // policy agent: this decision's evaluations by slot
  DevBuf<int32_t> rec_action, rec_n_legal;       // the side's decisions [G][max_moves]
  DevBuf<float> rec_prob;
  // nz_scs_agent_record: the policy agent's evaluations of chosen matches
  DevBuf<int32_t> hook_slot, hook_count;
  DevBuf<uint64_t> hook_digest;
  DevBuf<float> hook_probs, hook_value;
  int32_t hook_slots = 0, hook_cap = 0;
  // what a side of `kind` needs (an MCTS side: nothing); the hook's arrays are nz_scs_agent_record's
  bool ensure(int kind, size_t G, size_t M, size_t A) {
    if (kind == NZ_AGENT_MCTS) return true;
    if (kind == NZ_AGENT_RANDOM && !(seeds.ensure(G) && mt_keys.ensure(G * 624) && mt_pos.ensure(G))) return false;
    if (kind == NZ_AGENT_POLICY && !(count.ensure(1) && probs.ensure(G * A) && value.ensure(G))) return false;
    return rec_action.ensure(G * M) && rec_n_legal.ensure(G * M) && rec_prob.ensure(G * M);
  }
  void bind(AgentSide& s) const {
    s.probs = probs.get(); s.value = value.get(); s.count = count.get(); s.mt_keys = mt_keys.get(); s.mt_pos = mt_pos.get();
    s.rec_action = rec_action.get(); s.rec_n_legal = rec_n_legal.get(); s.rec_prob = rec_prob.get();
    s.hook_slot = hook_slots > 0 ? hook_slot.get() : nullptr; s.hook_cap = hook_cap; s.hook_count = hook_count.get();
    s.hook_digest = hook_digest.get(); s.hook_probs = hook_probs.get(); s.hook_value = hook_value.get();
  }
};

struct AgentBufs {                // nz_scs_agent_match_play
  AgentSideBufs side[2];
  // the forced actions of end_move [G], each match's evaluation slot [G] and error word [G], live matches and flags [3]
  DevBuf<int32_t> forced, slot, err, state;
  DevBuf<uint64_t> digest;        // [G][2]
  DevBuf<int64_t> tally;          // [8]
  PinnedBuf<int32_t> pinned;
  int32_t kinds[2] = {-1, -1};    // of the last round; -1: none was played
  bool ensure(const int kind[2], size_t G, size_t M, size_t A) {
    return side[0].ensure(kind[0], G, M, A) && side[1].ensure(kind[1], G, M, A) && forced.ensure(G) && slot.ensure(G) && err.ensure(G) && state.ensure(3) &&
           digest.ensure(G * 2) && tally.ensure(8) && pinned.ensure(3);
  }
};

struct OpeningBufs {              // nz_scs_search_reset_to, nz_scs_openings_draw / _expand (grown, never shrunk)
  DevBuf<int32_t> actions, n_plies, err;         // the matches' prefixes [G][max_plies], their lengths and error words [G]
  DevBuf<uint32_t> seeds;                        // draw: [G]
  DevBuf<int32_t> counts, offsets, children;     // expand: per prefix [n], the child prefixes [total][depth + 1]
  DevBuf<uint64_t> keys;                         // expand: [total][2]
  DevBuf<float> planes;                          // expand: a position's planes per prefix [n][channels][tiles]
};

}  // namespace

struct nz_scs_search {
  int device = 0, n_games = 0;
  nz_search_cfg cfg;
  ScsRules host_rules;
  SearchParams p;
  std::string error;
  CreateBufs made;
  PlayBufs play;                              // (the library's move loop)
  int64_t waves = 0;
  // nz_scs_search_play_round
  RoundBufs round_bufs;
  RoundStore round{};
  int64_t round_games = 0;
  // inference cache (nz_scs_search_cache)
  CacheBufs cache;
  int32_t cache_bits = 0, cache_wave = 0;
  int64_t cache_entries = 0;
  int cache_route = 0;                        // which route filled the table (1 wave by wave, 2 persistent); they do not mix
  // persistent route (persist_kernel): -1 follow the default (on where the network has a per-wavefront form), 0 off, 1 on
  int persist_mode = -1;
  int persist_used = 0;                       // the last play ran on it
  void (*persist_fn)(SearchParams, PersistArgs) = nullptr;     // the kernel variant of the last play
  bool persist_profile = false;               // HIP events around every persist_kernel launch (nz_scs_search_persist_profile)
  Event ev_p0, ev_p1;
  double persist_ms = 0.0;
  int64_t persist_launches = 0, persist_mfmas = 0, persist_flops = 0;
  std::string persist_why;                    // why not
  PersistArgs pq{};
  RecordBufs rec;
  int32_t rec_slots = 0;
  // per-game maps and streams of the next plays (nz_scs_search_set_games)
  GameRows rows;
  int64_t n_game_rows = 0;                    // rows in use; 0: the description's one map
  std::vector<nz_rng*> game_streams;          // [n_game_rows] or empty: streams from the seeds
  // nz_scs_search_draw_games: what a game draws and the last draw
  bool draw_set = false;
  ScsDrawSpec draw{};
  DrawBufs drawn;
  int64_t n_drawn = 0;                        // games of the last draw; 0 when the games were set otherwise
  MatchBufs match;
  const nz_scs_search* match_peer = nullptr;    // agent 2 of the last round (compared, never followed)
  AgentBufs agents;
  OpeningBufs openings;
};

namespace {
thread_local std::string g_err;
nz_status sfail(nz_scs_search* h, nz_status code, const char* fmt, ...) {
  char buf[384];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) h->error = buf; else g_err = buf;
  return code;
}
#define S_HIP(h, call)                                                                            \
  do {                                                                                            \
    hipError_t e__ = (call);                                                                      \
    if (e__ != hipSuccess) return sfail((h), NZ_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e__)); \
  } while (0)
// (bit 64 is the match check's: match_live_kernel reports "the engines no longer hold the same game" in the same word)
constexpr const char* FLAG_TEXT = "1 arena full, 2 visit table/path too short, 4 move ended before its search, 8 forced action is not legal, "
                                  "16 more legal actions than the bound computed at create, 32 game longer than that bound, "
                                  "128 the position has no legal action";
// what a check appends to its message when flag 128 is set: the first game that reached such a position and its decision number
std::string dead_end_text(nz_scs_search* h, int32_t flag, hipStream_t s) {
  if (!(flag & 128)) return "";
  int32_t at[2] = {-1, -1};
  if (hipMemcpyAsync(at, h->p.error_flag + 1, sizeof(at), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return "";
  char buf[128];
  snprintf(buf, sizeof(buf), "; game %d, decision %d: the position has no legal action and the game is not over", at[0], at[1]);
  return buf;
}
// the (leaf, active, cache hit) counter pointers at rest: the first triple, zeroed by the host (a wave-by-wave play leaves the last wave's)
void rest_counters(nz_scs_search* h) {
  int32_t* const counters = h->made.leaf_count.get();
  h->p.leaf_count = counters; h->p.active_count = counters + 1; h->p.hit_count = counters + 2;
  h->p.clear_counters = nullptr;
}
nz_status check_flag(nz_scs_search* h, hipStream_t s) {
  int32_t f = 0;
  S_HIP(h, hipMemcpyAsync(&f, h->p.error_flag, sizeof(f), hipMemcpyDeviceToHost, s));
  S_HIP(h, hipStreamSynchronize(s));
  if (f) return sfail(h, NZ_ERR_OVERFLOW, "device check failed (flag %d: %s%s)", f, FLAG_TEXT, dead_end_text(h, f, s).c_str());
  return NZ_OK;
}
// What nz_scs_search_reset_to refuses before any launch (nuzero_amd.scs_positions.check_openings is its twin); false: the
// message is in the handle.  NULL openings and max_plies == 0 are the plain reset.
bool openings_ok(nz_scs_search* h, const nz_scs_openings* o) {
  if (!o || o->max_plies == 0) return true;
  const int G = h->n_games, P = o->max_plies, A = h->p.num_actions;
  if (!o->actions) return sfail(h, NZ_ERR_ARG, "openings without actions") == NZ_OK;
  if (P < 0 || P > h->p.max_moves)
    return sfail(h, NZ_ERR_ARG, "openings of %d plies: 0 .. %d (the decisions a game's records hold)", P, h->p.max_moves) == NZ_OK;
  for (int g = 0; g < G; ++g) {
    const int np = o->n_plies ? o->n_plies[g] : P;
    if (np < 0 || np > P)
      return sfail(h, NZ_ERR_ARG, "match %d: an opening of %d plies, the openings hold 0 .. %d (ply %d is not there)", g, np, P,
                   np < 0 ? np : P) == NZ_OK;
    for (int ply = 0; ply < np; ++ply) {
      const int a = o->actions[(size_t)g * P + ply];
      if (a < 0 || a >= A) return sfail(h, NZ_ERR_ARG, "match %d, ply %d: action %d outside 0 .. %d", g, ply, a, A - 1) == NZ_OK;
    }
  }
  return true;
}
const char* opening_reason(int32_t e) {
  switch (nz::opening_err_reason(e)) {
    case nz::OPENING_ERR_ILLEGAL: return "the action is not legal in this position";
    case nz::OPENING_ERR_GAME_OVER: return "the game was over before the prefix ended";
    case nz::OPENING_ERR_LENGTH: return "the prefix runs past the decisions the records hold";
    case nz::OPENING_ERR_NO_LEGAL: return "a live position without a legal action";
    case nz::OPENING_ERR_CAP: return "the randint rejection cap was reached";
  }
  return "unknown";
}
nz::OpeningGames opening_games(const nz_scs_search* h) {
  return nz::OpeningGames{h->p.rules, h->p.rules_row, h->p.num_actions};
}
}  // namespace

extern "C" {

const char* nz_scs_search_last_error(const nz_scs_search* h) { return h ? h->error.c_str() : g_err.c_str(); }

nz_status nz_scs_search_create(nz_scs_search** out, const nz_scs_desc* d, const nz_search_cfg* cfg, int32_t n_games,
                               int32_t nodes_per_game, int32_t device) {
  if (!out || !d || !cfg) return sfail(nullptr, NZ_ERR_ARG, "null argument");
  *out = nullptr;
  if (n_games <= 0 || cfg->mcts_simulations <= 0 || (nodes_per_game > 0 && nodes_per_game < 4))
    return sfail(nullptr, NZ_ERR_ARG, "bad sizes");
  if (!cfg->keep_subtree) return sfail(nullptr, NZ_ERR_ARG, "keep_subtree = False is not supported (Gamer.py:78-79)");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
    return sfail(nullptr, NZ_ERR_HIP, "no HIP device %d (no CPU fallback)", device);
  nz_scs_search* h = new nz_scs_search;
  h->device = device;
  h->n_games = n_games;
  h->cfg = *cfg;
  std::string err;
  // (a description it accepts has at most SCS_MAX_PLANES action planes: what the side kernels' legal masks hold, scs_wave.hpp)
  if (!scs_fill_rules(d, &h->host_rules, &err)) { delete h; return sfail(nullptr, NZ_ERR_ARG, "%s", err.c_str()); }
  if (h->host_rules.planes * h->host_rules.tiles > MAX_ACTIONS) { delete h; return sfail(nullptr, NZ_ERR_ARG, "too many actions"); }
  (void)hipSetDevice(device);
  SearchParams& p = h->p;
  memset(&p, 0, sizeof(p));
  p.n_games = n_games;

  p.sims = cfg->mcts_simulations;
  p.training = cfg->training;
  p.softmax_moves = cfg->number_of_softmax_moves;
  p.negate_player = 2;                       // Explorer.py:124; SCS players are 0 and 1
  {   // what the records must hold, from the game description (the reference has no limits at all):
      //   decisions per game: one placement per unit, then per turn and unit at most ceil(movement / cheapest tile)
      //     steps + 1 "end movement", 1 "end fighting" or 1 target choice, 1 selection as attacker, 1 confirmation
      //   legal actions per position: scs_children_bound (scs_dev.hpp)
    const ScsRules& R = h->host_rules;
    int min_cost = 1 << 30;
    for (int t = 0; t < R.tiles; ++t) min_cost = std::min(min_cost, (int)R.cost[t]);
    if (min_cost < 1) { delete h; return sfail(nullptr, NZ_ERR_ARG, "a terrain with movement cost < 1 makes a game's length unbounded"); }
    long long moves = R.n_units;
    for (int u = 0; u < R.n_units; ++u) moves += (long long)R.turns * ((R.u_mov[u] + min_cost - 1) / min_cost + 4);
    const int children = scs_children_bound(R);
    if (children > MAXC_LIMIT) {
      delete h;
      return sfail(nullptr, NZ_ERR_ARG, "this game can have %d legal actions in one position; the search kernels hold %d "
                                        "children per node", children, MAXC_LIMIT);
    }
    if (moves > 32000) { delete h; return sfail(nullptr, NZ_ERR_ARG, "a game of this description can last %lld decisions (limit 32000)", moves); }
    p.maxc = (children + 63) / 64 * 64;
    p.max_moves = (int32_t)moves + 8;
  }
  const int MAX_MOVES = p.max_moves, MAXC = p.maxc;
  // Tree arena: two halves per game (compact_kernel copies the kept subtree into the other half at every re-root), so a
  // half holds the kept subtree plus one move's expansions.  Default: 2.5 x the children bound per simulation (160 nodes
  // for up to 64 children: what every configuration measured so far needed several times over); a full half is
  // reported (NZ_ERR_OVERFLOW), never silent.
  if (nodes_per_game <= 0) nodes_per_game = 2 * (1 + cfg->mcts_simulations * (5 * MAXC / 2));
  p.cap = nodes_per_game & ~1;
  p.half_cap = p.cap / 2;
  p.tab_len = cfg->mcts_simulations * MAX_MOVES + 2;
  p.max_path = std::max(MAX_MOVES + 8, 64);   // one tree level per game decision (at least a lane each: wave_kernel reads path[lane])
  {   // numpy's pairwise_sum over num_actions float32 entries (np.sum in Explorer.py:169) as a block program
    const int A = h->host_rules.planes * h->host_rules.tiles;
    p.num_actions = A;
    p.pw_blocks = 0;
    bool fits = true;
    struct Rec {
      static void build(SearchParams& q, int lo, int hi, bool& ok) {
        const int n = hi - lo;
        if (n <= 128) {
          if (q.pw_blocks >= 48) { ok = false; return; }
          q.pw_hi[q.pw_blocks] = (uint16_t)hi;
          q.pw_be[q.pw_blocks] = (uint16_t)(n < 8 ? lo : lo + (n - n % 8));
          q.pw_merge[q.pw_blocks] = 0;
          ++q.pw_blocks;
          return;
        }
        int n2 = n / 2;
        n2 -= n2 % 8;
        build(q, lo, lo + n2, ok);
        build(q, lo + n2, hi, ok);
        if (ok) q.pw_merge[q.pw_blocks - 1] += 1;
      }
    };
    Rec::build(p, 0, A, fits);
    if (!fits) { nz_scs_search_destroy(h); return sfail(nullptr, NZ_ERR_ARG, "too many actions for the pairwise-sum program"); }
  }
  p.terminal_budget = 1 << 30;
  p.frac = cfg->root_exploration_fraction;
  p.one_minus_frac = 1.0 - cfg->root_exploration_fraction;
  p.value_factor = cfg->value_factor;
  p.eps_softmax = cfg->epsilon_softmax_exploration;
  p.eps_random = cfg->epsilon_random_exploration;
  if (!h->made.ensure(p)) { nz_scs_search_destroy(h); return sfail(nullptr, NZ_ERR_HIP, "device allocation failed"); }
  h->rows.bind(p, h->made.rules.get(), false);
  std::vector<double> hb(p.tab_len), hs(p.tab_len);
  for (int n = 0; n < p.tab_len; ++n) {      // Explorer.py:103-112 with the host libm
    hb[n] = std::log(((double)n + cfg->pb_c_base + 1.0) / cfg->pb_c_base) + cfg->pb_c_init;
    hs[n] = std::sqrt((double)n);
  }
  if (hipMemcpy(h->made.rules.get(), &h->host_rules, sizeof(ScsRules), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->made.bias_tab.get(), hb.data(), hb.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->made.sqrt_tab.get(), hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    nz_scs_search_destroy(h);
    return sfail(nullptr, NZ_ERR_HIP, "upload failed");
  }
  rest_counters(h);
  (void)hipMemset(p.counters, 0, 16 * sizeof(int64_t));      // (the reset leaves the cache's three alone)
  hipLaunchKernelGGL(search_reset_kernel, dim3((n_games + 127) / 128), dim3(128), 0, nullptr, p);
  if (hipDeviceSynchronize() != hipSuccess) { nz_scs_search_destroy(h); return sfail(nullptr, NZ_ERR_HIP, "reset failed"); }
  *out = h;
  return NZ_OK;
}

void nz_scs_search_destroy(nz_scs_search* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  for (nz_rng* r : h->game_streams) nz_rng_destroy(r);
  delete h;
}

nz_status nz_scs_search_reset(nz_scs_search* h, void* stream) {
  if (!h) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(search_reset_kernel, dim3((h->n_games + 127) / 128), dim3(128), 0, (hipStream_t)stream, h->p);
  S_HIP(h, hipGetLastError());
  return NZ_OK;
}

nz_status nz_scs_search_root_children(nz_scs_search* h, int32_t* out_dev, void* stream) {
  if (!h || !out_dev) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(root_children_kernel, dim3((h->n_games + 127) / 128), dim3(128), 0, (hipStream_t)stream, h->p, out_dev);
  S_HIP(h, hipGetLastError());
  return NZ_OK;
}

// Test hook: the legal masks the searches stored with their pending leaves, one row of `*words_host` 32-bit words per game
// (action a is bit a & 31 of word a >> 5; all zero: a live position without a legal action).  masks_dev may be NULL (the
// row length alone).  A row is meaningful between nz_scs_search_select and nz_scs_search_expand for the games of leaf_game.
nz_status nz_scs_search_leaf_masks(nz_scs_search* h, uint32_t* masks_dev, int32_t* words_host, void* stream) {
  if (!h) return NZ_ERR_ARG;
  if (words_host) *words_host = MASK_WORDS;
  if (!masks_dev) return NZ_OK;
  S_HIP(h, hipSetDevice(h->device));
  S_HIP(h, hipMemcpyAsync(masks_dev, h->p.leaf_mask, (size_t)h->n_games * MASK_WORDS * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
  return NZ_OK;
}

nz_status nz_scs_search_status(nz_scs_search* h, int32_t* status_dev, void* stream) {
  if (!h || !status_dev) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(search_status_kernel, dim3((h->n_games + 127) / 128), dim3(128), 0, (hipStream_t)stream, h->p, status_dev);
  S_HIP(h, hipGetLastError());
  return NZ_OK;
}

nz_status nz_scs_search_begin_move(nz_scs_search* h, const double* noise_dev, void* stream) {
  if (!h) return NZ_ERR_ARG;
  if (h->cfg.training && !noise_dev) return sfail(h, NZ_ERR_ARG, "training search needs noise");
  S_HIP(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(begin_move_kernel, dim3(h->n_games), dim3(64), 0, (hipStream_t)stream, h->p, noise_dev);
  S_HIP(h, hipGetLastError());
  return NZ_OK;
}

nz_status nz_scs_search_select(nz_scs_search* h, float* images_dev, int32_t* leaf_game_dev, int32_t* n_leaves_host,
                               void* stream) {
  if (!h || !images_dev || !leaf_game_dev || !n_leaves_host) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  S_HIP(h, hipMemsetAsync(h->p.leaf_count, 0, 3 * sizeof(int32_t), s));
  h->p.c_bits = 0;                            // the cache lives in the library's own move loop (nz_scs_search_play)
  h->p.terminal_budget = 1 << 30;             // run on until a leaf needs an evaluation, as this API promises
  h->p.image_row_stride = 0;                  // NCHW images for the caller
  h->p.clear_counters = nullptr;
  hipLaunchKernelGGL(wave_kernel, dim3(h->n_games), dim3(64), 0, s, h->p, 2, (const float*)nullptr, (const float*)nullptr,
                     images_dev, leaf_game_dev);
  S_HIP(h, hipGetLastError());
  S_HIP(h, hipMemcpyAsync(n_leaves_host, h->p.leaf_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  S_HIP(h, hipStreamSynchronize(s));
  return check_flag(h, s);
}

nz_status nz_scs_search_expand(nz_scs_search* h, const float* probs_dev, const float* value_dev, void* stream) {
  if (!h || !probs_dev || !value_dev) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(wave_kernel, dim3(h->n_games), dim3(64), 0, (hipStream_t)stream, h->p, 1, probs_dev, value_dev,
                     (float*)nullptr, (int32_t*)nullptr);
  S_HIP(h, hipGetLastError());
  return NZ_OK;
}

nz_status nz_scs_search_end_move(nz_scs_search* h, const double* uniforms_dev, void* stream) {
  if (!h) return NZ_ERR_ARG;
  if (h->cfg.training && !uniforms_dev) return sfail(h, NZ_ERR_ARG, "training search needs uniforms");
  return nz_scs_search_apply(h, nullptr, uniforms_dev, stream);     // (no forced actions: every search chooses its own)
}

nz_status nz_scs_search_apply(nz_scs_search* h, const int32_t* actions_dev, const double* uniforms_dev, void* stream) {
  if (!h) return NZ_ERR_ARG;
  if (!actions_dev && h->cfg.training && !uniforms_dev) return sfail(h, NZ_ERR_ARG, "a training search choosing its own action needs uniforms");
  S_HIP(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(end_move_kernel, dim3((h->n_games + 63) / 64), dim3(64), 0, s, h->p, uniforms_dev, actions_dev);
  hipLaunchKernelGGL(compact_kernel, dim3(h->n_games), dim3(64), 0, s, h->p);
  S_HIP(h, hipGetLastError());
  return check_flag(h, s);
}

namespace {
__global__ void scs_last_actions_kernel(SearchParams p, int32_t* __restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.n_games) return;
  const int n = p.real[g].length;
  out[g] = n > 0 && n <= p.max_moves ? p.rec_action[(size_t)g * p.max_moves + n - 1] : -1;
}
}  // namespace

nz_status nz_scs_search_last_actions(nz_scs_search* h, int32_t* actions_dev, void* stream) {
  if (!h || !actions_dev) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(scs_last_actions_kernel, dim3((h->n_games + 127) / 128), dim3(128), 0, (hipStream_t)stream, h->p, actions_dev);
  S_HIP(h, hipGetLastError());
  return NZ_OK;
}

// Gamer.play_game for all games to the end with the network on the device too: the move loop of
// Training/Gamer.py:52-92 and Explorer.run_mcts, one simulation wave = [expand + select] kernel
// -> nz_boardnet_forward on the wave's leaves (batch size read from device memory).  The host
// only draws each move's random numbers (numpy RandomState streams, one per game, in the
// reference's order) and checks every few waves whether the move's searches are complete.
nz_status nz_scs_search_play(nz_scs_search* h, nz_boardnet* net, const uint32_t* seeds_host, void* stream) {
  return nz_scs_search_play_moves(h, net, seeds_host, 0, stream);
}

}  // extern "C"

namespace {
// a few host threads that live for one play call: every move hands them the same job (the games' random draws, a slice
// of the games each) -- starting and joining eight threads per move was a quarter of a millisecond of every move
class WorkerPool {
 public:
  explicit WorkerPool(int n) {
    for (int t = 0; t < n; ++t) threads_.emplace_back([this, t] { loop(t); });
  }
  ~WorkerPool() {
    { std::lock_guard<std::mutex> lk(m_); stop_ = true; ++generation_; }
    cv_.notify_all();
    for (std::thread& t : threads_) t.join();
  }
  int size() const { return (int)threads_.size(); }
  void run(const std::function<void(int)>& job) {            // job(thread index) on every thread; returns when all are done
    { std::lock_guard<std::mutex> lk(m_); job_ = &job; pending_ = (int)threads_.size(); ++generation_; }
    cv_.notify_all();
    std::unique_lock<std::mutex> lk(m_);
    done_.wait(lk, [this] { return pending_ == 0; });
  }
 private:
  void loop(int t) {
    long seen = 0;
    for (;;) {
      const std::function<void(int)>* job;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return generation_ != seen; });
        seen = generation_;
        if (stop_) return;
        job = job_;
      }
      (*job)(t);
      { std::lock_guard<std::mutex> lk(m_); if (--pending_ == 0) done_.notify_one(); }
    }
  }
  std::vector<std::thread> threads_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  const std::function<void(int)>* job_ = nullptr;
  long generation_ = 0;
  int pending_ = 0;
  bool stop_ = false;
};

// the round's store for `n` games
nz_status round_store(nz_scs_search* h, int64_t n) {
  if (n <= h->round_bufs.games) return NZ_OK;
  const bool ok = h->round_bufs.ensure(n, (size_t)h->n_games, h->p);
  h->round_bufs.bind(h->round);
  if (!ok) return sfail(h, NZ_ERR_HIP, "device allocation failed (round store for %lld games)", (long long)n);
  // unplayed moves' child rows are never written by archive_kernel: keep them defined
  const RoundStore& r = h->round;
  const size_t NMC = (size_t)n * h->p.max_moves * h->p.maxc;
  S_HIP(h, hipMemset(r.child_action, 0, NMC * 4)); S_HIP(h, hipMemset(r.child_visit, 0, NMC * 4));
  S_HIP(h, hipMemset(r.child_prior, 0, NMC * 8)); S_HIP(h, hipMemset(r.child_value_sum, 0, NMC * 8));
  return NZ_OK;
}

// The records of `games` games in `r` to the caller's device arrays `out` (any may be null), and the simulation and
// expansion counters to the host (nz_scs_search_export, nz_scs_search_export_round).
nz_status export_records(nz_scs_search* h, const RoundStore& r, size_t games, const RoundStore& out, int64_t* counters_host, hipStream_t s) {
  const size_t NM = games * h->p.max_moves, NMC = NM * h->p.maxc;
  auto copy = [s](auto* dst, const auto* src, size_t n) {
    return dst ? hipMemcpyAsync(dst, src, n * sizeof(*src), hipMemcpyDeviceToDevice, s) : hipSuccess;
  };
  S_HIP(h, copy(out.action, r.action, NM)); S_HIP(h, copy(out.tree_size, r.tree_size, NM)); S_HIP(h, copy(out.children, r.children, NM));
  S_HIP(h, copy(out.bias, r.bias, NM)); S_HIP(h, copy(out.root_value_sum, r.root_value_sum, NM));
  S_HIP(h, copy(out.child_action, r.child_action, NMC)); S_HIP(h, copy(out.child_visit, r.child_visit, NMC));
  S_HIP(h, copy(out.child_prior, r.child_prior, NMC)); S_HIP(h, copy(out.child_value_sum, r.child_value_sum, NMC));
  S_HIP(h, copy(out.status, r.status, games * 2));
  if (counters_host) {
    S_HIP(h, hipMemcpyAsync(counters_host, h->p.counters, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    S_HIP(h, hipStreamSynchronize(s));
  }
  return NZ_OK;
}

// the network's per-wavefront form as the persistent kernels read it
void persist_net_args(PersistArgs* q, const nz::WaveNet& wn) {
  q->prog = wn.prog; q->net_floats = wn.lds_floats; q->stage_off = wn.stage_off; q->stage_floats = wn.stage_floats;
  q->inp = wn.inp; q->in_channels = wn.in_channels;
  q->wave_bytes = PERSIST_GAME_BYTES + (wn.lds_floats * 4 + 15) / 16 * 16;
}

// What a play call settles before its first move: the network fits the game, the move loop's buffers exist, and the
// route -- persistent where the network has a per-wavefront form -- is chosen (nz_scs_search_play*, nz_scs_match_play).
struct PlayRoute {
  bool persist = false;
  size_t persist_lds = 0;
  float* net_rows = nullptr;                   // the leaf images go straight into the network's input rows
  int32_t row_stride = 0;
};

// The network fits the handle's game and holds a position of each of its games; its input rows.  agent = 1 / 2: the
// network of a scripted side of an agent match (the message says whose), 0: the searching network.
nz_status net_fits(nz_scs_search* h, nz_boardnet* net, int agent, float** net_rows, int32_t* row_stride) {
  const ScsRules& R = h->host_rules;
  char who[16] = "";
  if (agent) snprintf(who, sizeof(who), "agent %d: ", agent);
  int32_t nin = 0, npol = 0, nrows = 0, ncols = 0, nmax = 0;
  if (nz_boardnet_dims(net, &nin, &npol, &nrows, &ncols, &nmax) != NZ_OK) return sfail(h, NZ_ERR_ARG, "%sbad network handle", who);
  if (nin != R.channels || npol != R.planes || nrows != R.rows || ncols != R.cols)
    return sfail(h, NZ_ERR_ARG, "%snetwork is %d planes -> %d planes on %dx%d, the game needs %d -> %d on %dx%d", who, nin, npol,
                 nrows, ncols, R.channels, R.planes, R.rows, R.cols);
  if (nmax < h->n_games) return sfail(h, NZ_ERR_ARG, "%snetwork max_batch %d < %d %s", who, nmax, h->n_games, agent ? "matches" : "games");
  if (nz_boardnet_input_rows(net, net_rows, row_stride) != NZ_OK) return sfail(h, NZ_ERR_ARG, "%sbad network handle", who);
  return NZ_OK;
}

nz_status play_prepare(nz_scs_search* h, nz_boardnet* net, PlayRoute* route, void* stream) {
  const int G = h->n_games;
  const int MAXC = h->p.maxc;
  const ScsRules& R = h->host_rules;
  const int A = R.planes * R.tiles;
  if (nz_status st = net_fits(h, net, 0, &route->net_rows, &route->row_stride)) return st;
  const bool bufs = h->play.ensure((size_t)G, (size_t)A, (size_t)MAXC);
  h->play.bind(h->p);
  if (!bufs) return sfail(h, NZ_ERR_HIP, "device allocation failed");
  // the persistent route: the network must have a per-wavefront form
  bool& persist = route->persist;
  size_t& persist_lds = route->persist_lds;
  h->persist_used = 0;
  {
    static const int env_mode = getenv("NZ_SCS_PERSIST") ? atoi(getenv("NZ_SCS_PERSIST")) : -1;       // A/B experiments
    const int mode = h->persist_mode >= 0 ? h->persist_mode : env_mode;
    nz::WaveNet wn{};
    std::string why;
    if (mode == 0) h->persist_why = "switched off";
    else if (!nz::boardnet_wave_program(net, &wn, &why)) h->persist_why = why;
    else {
      PersistArgs& q = h->pq;
      persist_net_args(&q, wn);
      h->persist_mfmas = wn.mfmas; h->persist_flops = wn.flops;
      q.rules_per_game = h->n_game_rows > 0 ? 1 : 0;
      persist_lds = (size_t)(q.rules_per_game ? PERSIST_GAMES : 1) * PERSIST_RULES_BYTES + (size_t)PERSIST_GAMES * q.wave_bytes;
      if (persist_lds > 160 * 1024) h->persist_why = "four games' blocks do not fit in LDS";
      else {
        h->persist_fn = persist_pick(wn.hex != 0, h->p.maxc <= 64, wn.precision);
        const hipError_t e = hipFuncSetAttribute((const void*)h->persist_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)persist_lds);
        if (e != hipSuccess) { (void)hipGetLastError(); h->persist_why = "hipFuncSetAttribute failed"; }
        else { persist = true; h->persist_why.clear(); }
      }
      if (persist) h->persist_used = wn.hex ? 2 : 1;
    }
    if (mode == 1 && !persist) return sfail(h, NZ_ERR_STATE, "persistent route requested but not available: %s", h->persist_why.c_str());
    if (h->rec_slots > 0 && !persist) return sfail(h, NZ_ERR_STATE, "leaf recording needs the persistent route: %s", h->persist_why.c_str());
  }
  if (h->cache_bits > 0 && h->cache_route != (persist ? 2 : 1)) {
    // the two routes keep their entries differently (check words / writer serial numbers): a table filled by the other
    // one starts empty
    if (h->cache_route != 0) {
      const size_t n = (size_t)h->cache_entries;
      S_HIP(h, hipMemsetAsync(h->p.c_id, 0, n * 2 * sizeof(uint64_t), (hipStream_t)stream));
      S_HIP(h, hipMemsetAsync(h->p.c_writer, 0, n * sizeof(int32_t), (hipStream_t)stream));
      S_HIP(h, hipMemsetAsync(h->p.c_check, 0, n * sizeof(uint64_t), (hipStream_t)stream));
    }
    h->cache_route = persist ? 2 : 1;
  }
  return NZ_OK;
}

// The search of one move for every live game of `h`, enqueued on `s`: begin_move, then the persistent kernel (one
// launch) or the simulation waves (the host waits for the move's last ones).  end_move is the caller's.
nz_status search_move(nz_scs_search* h, nz_boardnet* net, const PlayRoute& route, hipStream_t s) {
  const int G = h->n_games;
  int32_t* const counters = h->made.leaf_count.get();
  float *const probs = h->play.probs.get(), *const value = h->play.value.get();
  hipLaunchKernelGGL(begin_move_kernel, dim3(G), dim3(64), 0, s, h->p, h->play.noise.get());
  h->p.image_row_stride = route.row_stride;
  S_HIP(h, hipMemsetAsync(counters, 0, 6 * sizeof(int32_t), s));
  h->p.c_bits = h->cache_bits;
  h->p.terminal_budget = 1;                  // measured best (bench_scs.py: 1 -> 308 games/s, 16 -> 259, unbounded -> 226)
  if (route.persist) {                       // the whole move's search of every game: one launch
    if (h->persist_profile) {
      if (!h->ev_p0.create() || !h->ev_p1.create()) return sfail(h, NZ_ERR_HIP, "hipEventCreate failed");
      S_HIP(h, hipEventRecord(h->ev_p0.get(), s));
    }
    const dim3 pgrid((G + PERSIST_GAMES - 1) / PERSIST_GAMES);
    hipLaunchKernelGGL(h->persist_fn, pgrid, dim3(PERSIST_THREADS), route.persist_lds, s, h->p, h->pq);
    S_HIP(h, hipGetLastError());
    ++h->waves;
    if (h->persist_profile) S_HIP(h, hipEventRecord(h->ev_p1.get(), s));
    return NZ_OK;
  }
  const int sims = h->cfg.mcts_simulations;
  bool poll_pending = false;
  int32_t* const active_pinned = h->play.active.get();
  const hipEvent_t ev_poll = h->play.ev_poll.get();
  for (int w = 0;; ++w) {
    // two (leaf, active) counter pairs: wave w counts into pair w & 1 and zeroes the other one for wave w + 1
    h->p.leaf_count = counters + 3 * (w & 1);
    h->p.active_count = h->p.leaf_count + 1;
    h->p.hit_count = h->p.leaf_count + 2;
    h->p.clear_counters = counters + 3 * ((w + 1) & 1);
    h->p.c_wave = ++h->cache_wave;
    h->p.c_hit_base = G * (1 + (w & 1));
    hipLaunchKernelGGL(wave_kernel, dim3(G), dim3(64), 0, s, h->p, w ? 3 : 2, probs, value, route.net_rows, h->play.leaf_game.get());
    ++h->waves;
    if (w >= sims - 1) {                       // the move's last waves: wait for the count of games still searching
      int32_t active = 0;
      S_HIP(h, hipMemcpyAsync(&active, h->p.active_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      S_HIP(h, hipStreamSynchronize(s));
      if (active == 0) break;
      if (w > sims + 2) return sfail(h, NZ_ERR_STATE, "internal: a move's searches did not finish in %d waves", w);
    } else if ((w & 7) == 7) {
      // every game may have finished early (simulations that end in terminal leaves do not wait for a wave): the count
      // is copied to pinned memory and looked at eight waves later -- no wait, the GPU is never left without work; the
      // waves launched in between find nothing to do
      if (poll_pending && hipEventQuery(ev_poll) == hipSuccess) {
        poll_pending = false;
        if (*active_pinned == 0) break;
      }
      if (!poll_pending) {
        S_HIP(h, hipMemcpyAsync(active_pinned, h->p.active_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        S_HIP(h, hipEventRecord(ev_poll, s));
        poll_pending = true;
      }
    }
    if (nz_boardnet_forward_rows(net, G, h->p.leaf_count, nullptr, probs, value, (void*)s) != NZ_OK)
      return sfail(h, NZ_ERR_HIP, "network: %s", nz_boardnet_last_error(net));
    if (h->cache_bits > 0)                   // the leaves the network just evaluated enter the table (KeylessCache.put)
      hipLaunchKernelGGL(cache_put_kernel, dim3(G), dim3(64), 0, s, h->p, h->p.leaf_count);
  }
  if (poll_pending) S_HIP(h, hipEventSynchronize(ev_poll));     // (long done: the move's last waves were waited for)
  return NZ_OK;
}

// The library's move loop.  n_round == n_games: one game per slot (nz_scs_search_play_moves).  n_round > n_games: a round
// of n_round games over the engine's slots -- a slot whose game has ended hands its records to the round's store and
// starts the next game of the round (nz_scs_search_play_round); game i of the round is seeded with seeds_host[i]
// wherever and whenever it runs, so the round's games do not depend on the number of slots.
nz_status play_impl(nz_scs_search* h, nz_boardnet* net, const uint32_t* seeds_host, int64_t n_round, int32_t max_moves,
                    void* stream) {
  if (!h || !net || (h->cfg.training && !seeds_host && h->game_streams.empty())) return sfail(h, NZ_ERR_ARG, "null argument");
  const bool refill = n_round > h->n_games;
  if (n_round < h->n_games) return sfail(h, NZ_ERR_ARG, "a round has at least one game per slot (%d)", h->n_games);
  if (refill && max_moves > 0) return sfail(h, NZ_ERR_ARG, "max_moves applies to one game per slot only");
  S_HIP(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const int G = h->n_games;
  const int MAX_MOVES = h->p.max_moves, MAXC = h->p.maxc;
  PlayRoute route;
  if (nz_status pst = play_prepare(h, net, &route, stream)) return pst;
  std::vector<nz_rng*> rngs;
  struct RngGuard {
    std::vector<nz_rng*>& v;
    ~RngGuard() { for (nz_rng* r : v) nz_rng_destroy(r); }
  } guard{rngs};
  const bool own_games = h->n_game_rows > 0;       // per-game maps (and streams) from nz_scs_search_set_games
  if (own_games && n_round > h->n_game_rows)
    return sfail(h, NZ_ERR_ARG, "%lld games in the round, %lld set with nz_scs_search_set_games", (long long)n_round, (long long)h->n_game_rows);
  // the stream of game i of the round: where its map's draws left it (set_games), else RandomState(seeds_host[i])
  auto new_stream = [&](int64_t i) -> nz_rng* {
    if (!h->game_streams.empty()) return nz_rng_clone(h->game_streams[(size_t)i]);
    return nz_rng_create(seeds_host[i]);
  };
  if (h->cfg.training)
    for (int g = 0; g < G; ++g) rngs.push_back(new_stream(g));
  std::vector<int32_t> rules_rows(G);
  if (own_games) {
    for (int g = 0; g < G; ++g) rules_rows[g] = g;
    S_HIP(h, hipMemcpyAsync(h->rows.row.get(), rules_rows.data(), (size_t)G * sizeof(int32_t), hipMemcpyHostToDevice, (hipStream_t)stream));
    S_HIP(h, hipStreamSynchronize((hipStream_t)stream));
  }
  PinnedBuf<int32_t> status, nchild;
  PinnedBuf<double> noise, uni;
  if (!status.ensure((size_t)G * 7) || !nchild.ensure(G) || !noise.ensure((size_t)G * MAXC) || !uni.ensure((size_t)G * 3))
    return sfail(h, NZ_ERR_HIP, "host allocation failed");
  const int n_thr = h->cfg.training && G >= 256 ? std::min<int>(8, std::max<unsigned>(1u, std::thread::hardware_concurrency())) : 0;
  WorkerPool pool(n_thr);
  nz_status st = nz_scs_search_reset(h, stream);
  if (st != NZ_OK) return st;
  h->waves = 0;
  h->round_games = 0;
  std::vector<int32_t> slot_game(G), to_record(G), restart(G);     // round bookkeeping: the game each slot is playing
  int64_t next_game = G;
  for (int g = 0; g < G; ++g) slot_game[g] = g;
  if (refill) {
    st = round_store(h, n_round);
    if (st != NZ_OK) return st;
  }
  int32_t *const status_dev = h->play.status.get(), *const nchild_dev = h->play.nchild.get();
  int32_t *const to_record_dev = h->round_bufs.to_record.get(), *const restart_dev = h->round_bufs.restart.get();
  const dim3 grid1((G + 127) / 128), block1(128);
  const int64_t move_limit = refill ? (int64_t)MAX_MOVES * ((n_round + G - 1) / G + 1)
                                    : (max_moves > 0 && max_moves < MAX_MOVES ? max_moves : MAX_MOVES);
  for (int64_t move = 0; move < move_limit; ++move) {
    hipLaunchKernelGGL(search_status_kernel, grid1, block1, 0, s, h->p, status_dev);
    if (h->cfg.training) hipLaunchKernelGGL(root_children_kernel, grid1, block1, 0, s, h->p, nchild_dev);
    S_HIP(h, hipMemcpyAsync(status.get(), status_dev, status.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (h->cfg.training)
      S_HIP(h, hipMemcpyAsync(nchild.get(), nchild_dev, nchild.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    S_HIP(h, hipStreamSynchronize(s));
    if (refill) {
      bool archive = false, restarted = false;
      for (int g = 0; g < G; ++g) {
        to_record[g] = -1;
        restart[g] = 0;
        if (!status[(size_t)g * 7 + 4] || slot_game[g] < 0) continue;
        to_record[g] = slot_game[g];                 // the slot's game is over: its records go to the round's store
        archive = true;
        if (next_game < n_round) {                    // and the slot starts the round's next game
          slot_game[g] = (int32_t)next_game;
          if (h->cfg.training) {
            nz_rng_destroy(rngs[g]);
            rngs[g] = new_stream(next_game);
          }
          rules_rows[g] = (int32_t)next_game;          // (its own map, where the games have them)
          ++next_game;
          restart[g] = 1;
          restarted = true;
        } else {
          slot_game[g] = -1;
        }
      }
      if (archive) {
        S_HIP(h, hipMemcpyAsync(to_record_dev, to_record.data(), (size_t)G * sizeof(int32_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(archive_kernel, dim3(G), dim3(64), 0, s, h->p, h->round, to_record_dev);
      }
      if (restarted) {
        if (own_games)
          S_HIP(h, hipMemcpyAsync(h->rows.row.get(), rules_rows.data(), (size_t)G * sizeof(int32_t), hipMemcpyHostToDevice, s));
        S_HIP(h, hipMemcpyAsync(restart_dev, restart.data(), (size_t)G * sizeof(int32_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(restart_kernel, grid1, block1, 0, s, h->p, restart_dev);
        hipLaunchKernelGGL(search_status_kernel, grid1, block1, 0, s, h->p, status_dev);
        if (h->cfg.training) hipLaunchKernelGGL(root_children_kernel, grid1, block1, 0, s, h->p, nchild_dev);
        S_HIP(h, hipMemcpyAsync(status.get(), status_dev, status.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (h->cfg.training)
          S_HIP(h, hipMemcpyAsync(nchild.get(), nchild_dev, nchild.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      }
      if (archive) S_HIP(h, hipStreamSynchronize(s));     // the bookkeeping vectors are reused next move
    }
    bool any = false;
    for (int g = 0; g < G; ++g) any |= status[(size_t)g * 7 + 4] == 0;
    if (!any) break;
    if (h->cfg.training) {
      std::fill(noise.get(), noise.get() + noise.size(), 0.0);
      std::fill(uni.get(), uni.get() + uni.size(), 0.0);
      // (every game has its own stream: the draws of different games run on host threads side by side)
      auto draw = [&](int g0, int g1) {
        for (int g = g0; g < g1; ++g) {
          if (status[(size_t)g * 7 + 4]) continue;
          nz_rng* r = rngs[g];
          nz_rng_gamma(r, h->cfg.root_dist_alpha, h->cfg.root_dist_beta, nchild[g], &noise[(size_t)g * MAXC]);
          double* u = &uni[(size_t)g * 3];
          if (status[(size_t)g * 7 + 6] < h->cfg.number_of_softmax_moves) {
            u[2] = nz_rng_double(r);
          } else {
            u[0] = nz_rng_double(r);
            u[1] = nz_rng_double(r);
            if (u[0] < h->cfg.epsilon_softmax_exploration || u[1] < h->cfg.epsilon_random_exploration) u[2] = nz_rng_double(r);
          }
        }
      };
      if (n_thr <= 1) draw(0, G);
      else pool.run([&](int t) { draw((int)((int64_t)G * t / n_thr), (int)((int64_t)G * (t + 1) / n_thr)); });
      S_HIP(h, hipMemcpyAsync(h->play.noise.get(), noise.get(), noise.size() * sizeof(double), hipMemcpyHostToDevice, s));
      S_HIP(h, hipMemcpyAsync(h->play.uniforms.get(), uni.get(), uni.size() * sizeof(double), hipMemcpyHostToDevice, s));
    }
    st = search_move(h, net, route, s);
    if (st != NZ_OK) return st;
    st = nz_scs_search_end_move(h, h->play.uniforms.get(), stream);     // (synchronises)
    if (st != NZ_OK) return st;
    if (route.persist && h->persist_profile) {
      float ms = 0.f;
      S_HIP(h, hipEventElapsedTime(&ms, h->ev_p0.get(), h->ev_p1.get()));
      h->persist_ms += ms;
      ++h->persist_launches;
    }
  }
  rest_counters(h);
  if (refill) {
    for (int g = 0; g < G; ++g)
      if (slot_game[g] >= 0) return sfail(h, NZ_ERR_STATE, "internal: the round did not finish in %lld moves", (long long)move_limit);
    h->round_games = n_round;
  }
  return NZ_OK;
}
}  // namespace

extern "C" {

nz_status nz_scs_search_play_moves(nz_scs_search* h, nz_boardnet* net, const uint32_t* seeds_host, int32_t max_moves,
                                   void* stream) {
  return play_impl(h, net, seeds_host, h ? h->n_games : 0, max_moves, stream);
}

// A round of n_round >= n_games games over the engine's slots (see play_impl); read it with nz_scs_search_export_round.
nz_status nz_scs_search_play_round(nz_scs_search* h, nz_boardnet* net, const uint32_t* seeds_host, int64_t n_round,
                                   void* stream) {
  return play_impl(h, net, seeds_host, n_round, 0, stream);
}

// nz_scs_search_export for the last nz_scs_search_play_round with more games than slots: arrays of n_round rows, and
// status [n_round][2] = (length, terminal value) of every game.  (A round of exactly n_games games is read with
// nz_scs_search_export / nz_scs_search_status.)
nz_status nz_scs_search_export_round(nz_scs_search* h, int32_t* actions, int32_t* tree_size, int32_t* n_children,
                                     double* bias, double* root_value_sum, int32_t* child_action, int32_t* child_visit,
                                     double* child_prior, double* child_value_sum, int32_t* status2,
                                     int64_t* counters_host, void* stream) {
  if (!h) return NZ_ERR_ARG;
  if (h->round_games <= 0) return sfail(h, NZ_ERR_STATE, "no finished round of more games than slots");
  S_HIP(h, hipSetDevice(h->device));
  return export_records(h, h->round, (size_t)h->round_games,
                        RoundStore{actions, tree_size, n_children, child_action, child_visit, status2, bias, root_value_sum, child_prior, child_value_sum},
                        counters_host, (hipStream_t)stream);
}

// The reference's inference cache for the library's move loop (cache_choice "keyless" / "dict" of Gamer,
// Training/Gamer.py:20,53-55; KeylessCache.py:27-38: the table size is the largest power of two <= max_size).
// max_entries > 0: (re)allocate an empty table; 0: switch the cache off; < 0: empty the table, keep it.  Per-game maps
// (nz_scs_search_set_games) are part of the key: a leaf's key mixes its state's hash with its map row's digest.
nz_status nz_scs_search_cache(nz_scs_search* h, int64_t max_entries) {
  if (!h) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  S_HIP(h, hipDeviceSynchronize());
  SearchParams& p = h->p;
  const size_t A = (size_t)p.num_actions;
  if (max_entries >= 0) {
    h->cache = CacheBufs{};
    h->cache.bind(p);
    h->cache_bits = 0; h->cache_entries = 0;
    if (max_entries == 0) {                    // no table: nz_scs_search_cache_stats reports none, not the last one's
      S_HIP(h, hipMemset(p.counters + 8, 0, 3 * sizeof(int64_t)));
      return NZ_OK;
    }
    int bits = 0;
    while ((2ll << bits) <= max_entries && bits < 30) ++bits;          // closest power of two under max_entries
    if (bits == 0) bits = 1;
    const size_t n = (size_t)1 << bits;
    if (!h->cache.ensure(n, A)) return sfail(h, NZ_ERR_HIP, "cache allocation failed (%zu entries of %zu actions)", n, A);
    h->cache.bind(p);
    h->cache_bits = bits;
    h->cache_entries = (int64_t)n;
  }
  if (h->cache_bits > 0) {
    const size_t n = (size_t)h->cache_entries;
    S_HIP(h, hipMemset(p.c_id, 0, n * 2 * sizeof(uint64_t)));
    S_HIP(h, hipMemset(p.c_writer, 0, n * sizeof(int32_t)));
    S_HIP(h, hipMemset(p.c_check, 0, n * sizeof(uint64_t)));
    S_HIP(h, hipMemset(p.counters + 8, 0, 3 * sizeof(int64_t)));
    h->cache_wave = 0;
  }
  return NZ_OK;
}

// out4: hits, misses, entries in use, table size (Cache.get_hit_ratio / length / get_fill_ratio)
nz_status nz_scs_search_cache_stats(nz_scs_search* h, int64_t* out4_host) {
  if (!h || !out4_host) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  S_HIP(h, hipDeviceSynchronize());
  S_HIP(h, hipMemcpy(out4_host, h->p.counters + 8, 3 * sizeof(int64_t), hipMemcpyDeviceToHost));
  out4_host[3] = h->cache_entries;
  if (h->cache_bits > 0) {      // entries in use: counted on the table itself (the persistent route's writers keep no count)
    S_HIP(h, hipMemset(h->p.counters + 10, 0, sizeof(int64_t)));
    hipLaunchKernelGGL(cache_count_kernel, dim3(256), dim3(256), 0, nullptr, h->p.c_id, h->cache_entries, h->p.counters + 10);
    S_HIP(h, hipDeviceSynchronize());
    S_HIP(h, hipMemcpy(out4_host + 2, h->p.counters + 10, sizeof(int64_t), hipMemcpyDeviceToHost));
  }
  return NZ_OK;
}

// Diagnostic (library built with -DNZ_SCS_STAMPS; zeros otherwise): shader ticks summed over all games and waves
// since the last reset -- out6: expansion, rules copy, scratch clone, descent, leaf mask + image, terminal simulations.
nz_status nz_scs_search_phase_ticks(nz_scs_search* h, int64_t* out6_host) {
  if (!h || !out6_host) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  S_HIP(h, hipDeviceSynchronize());
  S_HIP(h, hipMemcpy(out6_host, h->p.counters + 2, 6 * sizeof(int64_t), hipMemcpyDeviceToHost));
  return NZ_OK;
}

// The persistent route of the library's move loop (persist_kernel).  enable: 1 require it (a play then fails where it is
// not available), 0 never use it, -1 the default (use it where it is available).  *used: whether the last play ran on it.
nz_status nz_scs_search_persistent(nz_scs_search* h, int32_t enable, int32_t* used) {
  if (!h) return NZ_ERR_ARG;
  if (enable >= -1 && enable <= 1) h->persist_mode = enable;
  if (used) *used = h->persist_used ? 1 : 0;
  return NZ_OK;
}

namespace {
// Back to the description's one map; the per-game buffers stay for the next rows.
void clear_games(nz_scs_search* h) {
  for (nz_rng* r : h->game_streams) nz_rng_destroy(r);
  h->game_streams.clear();
  h->n_game_rows = 0;
  h->n_drawn = 0;
  h->rows.bind(h->p, h->made.rules.get(), false);
}

// Slot g reads row g of the per-game rows (a refilled round leaves the slots on later rows).  A copy that waits: a
// caller whose stream may still read the rows waits for that stream first.
nz_status slots_read_own_rows(nz_scs_search* h) {
  std::vector<int32_t> ident(h->n_games);
  for (int g = 0; g < h->n_games; ++g) ident[g] = g;
  S_HIP(h, hipMemcpy(h->rows.row.get(), ident.data(), ident.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  return NZ_OK;
}

// The rows are in place: slot g plays row g, the plays read the per-game rows and digests.
nz_status use_game_rows(nz_scs_search* h, int64_t n, void* stream) {
  if (nz_status st = slots_read_own_rows(h)) return st;
  h->n_game_rows = n;
  h->rows.bind(h->p, h->made.rules.get(), true);
  return nz_scs_search_reset(h, stream);       // the slots' games start on their own maps (row g for slot g)
}
}  // namespace

// Every game of the next plays on its OWN map, as the reference builds a new game object -- and with a "Randomized"
// config a new map -- per game (Training/Gamer.py:52, SCS_Game.py:1678-1738).  Host arrays for n games (n >= the games of
// a round): terrain float32 [n][tiles][3] (attack modifier, defense modifier, cost), vp int32 [n][n_vp0 + n_vp1][2] (row,
// column); and, optionally, the random stream each game goes on with after its map's draws (numpy RandomState state:
// mt_keys uint32 [n][624], mt_pos int32 [n]; NULL: the plays' seeds make the streams).  n = 0: back to the description's
// one map.  Game i of a round reads row i whichever slot plays it.
nz_status nz_scs_search_set_games(nz_scs_search* h, int64_t n, const float* terrain_host, const int32_t* vp_host,
                                  const uint32_t* mt_keys_host, const int32_t* mt_pos_host) {
  if (!h || n < 0 || (n > 0 && (!terrain_host || !vp_host)) || ((mt_keys_host == nullptr) != (mt_pos_host == nullptr)))
    return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  S_HIP(h, hipDeviceSynchronize());
  clear_games(h);
  if (n == 0) return nz_scs_search_reset(h, nullptr);
  if (n < h->n_games) return sfail(h, NZ_ERR_ARG, "%lld games set, the engine plays %d at a time", (long long)n, h->n_games);
  const ScsRules& b = h->host_rules;
  const int T = b.tiles, nv = b.n_vp[0] + b.n_vp[1];
  std::vector<ScsRules> rows((size_t)n, b);
  for (int64_t i = 0; i < n; ++i) {
    nz::scs_apply_map(&rows[(size_t)i], terrain_host + (size_t)i * T * 3, vp_host + (size_t)i * nv * 2);
    for (int t = 0; t < T; ++t)
      if (rows[(size_t)i].cost[t] < 1) return sfail(h, NZ_ERR_ARG, "game %lld: a terrain with movement cost < 1", (long long)i);
  }
  std::vector<uint64_t> keys((size_t)n * 2);
  for (int64_t i = 0; i < n; ++i) scs_map_digest(rows[(size_t)i], &keys[(size_t)i * 2]);
  if (!h->rows.ensure((size_t)n, (size_t)h->n_games)) return sfail(h, NZ_ERR_HIP, "device allocation failed (%lld game descriptions)", (long long)n);
  S_HIP(h, hipMemcpy(h->rows.rules.get(), rows.data(), rows.size() * sizeof(ScsRules), hipMemcpyHostToDevice));
  S_HIP(h, hipMemcpy(h->rows.key.get(), keys.data(), keys.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  if (mt_keys_host)
    for (int64_t i = 0; i < n; ++i) {
      nz_rng* r = nz_rng_create_state(mt_keys_host + (size_t)i * 624, mt_pos_host[i], 0, 0.0);
      if (!r) return sfail(h, NZ_ERR_ARG, "game %lld: bad stream position %d", (long long)i, mt_pos_host[i]);
      h->game_streams.push_back(r);
    }
  return use_game_rows(h, n, nullptr);
}

// What a "Randomized" config draws per game (SCS_Game.py:1678-1738), checked against the description the engine was
// created with; NULL forgets it.  A refused spec leaves the one set before.
nz_status nz_scs_search_set_map_draw(nz_scs_search* h, const nz_scs_map_draw* spec) {
  if (!h) return NZ_ERR_ARG;
  if (!spec) {
    h->draw_set = false;
    return NZ_OK;
  }
  const ScsRules& b = h->host_rules;
  ScsDrawSpec d{};
  bool map = false, vps = false;
  for (int s = 0; s < 2; ++s) {
    const int o = spec->order[s];
    if (o != 0 && o != NZ_SCS_DRAW_MAP && o != NZ_SCS_DRAW_VP) return sfail(h, NZ_ERR_ARG, "unknown section %d in the draw order", o);
    if ((o == NZ_SCS_DRAW_MAP && map) || (o == NZ_SCS_DRAW_VP && vps)) return sfail(h, NZ_ERR_ARG, "a section drawn twice");
    map |= o == NZ_SCS_DRAW_MAP;
    vps |= o == NZ_SCS_DRAW_VP;
    d.order[s] = o;
  }
  if (!map && !vps) return sfail(h, NZ_ERR_ARG, "no randomized map or victory points: there is nothing to draw");
  if (map) {
    if (spec->n_types < 1 || spec->n_types > SCS_DRAW_MAX_TYPES || !spec->types || !spec->cdf)
      return sfail(h, NZ_ERR_ARG, "%d terrain types (1 to %d, with their cdf)", spec->n_types, SCS_DRAW_MAX_TYPES);
    d.n_types = spec->n_types;
    for (int i = 0; i < d.n_types; ++i) {
      for (int k = 0; k < 3; ++k) d.types[i][k] = spec->types[i * 3 + k];
      d.cdf[i] = spec->cdf[i];
      if (!(d.cdf[i] >= 0.0) || (i > 0 && d.cdf[i] < d.cdf[i - 1]))
        return sfail(h, NZ_ERR_ARG, "the terrain cdf is not a non-decreasing list of non-negative numbers");
    }
    if (d.cdf[d.n_types - 1] != 1.0) return sfail(h, NZ_ERR_ARG, "the terrain cdf does not end at 1");
  }
  if (vps) {
    for (int q = 0; q < 2; ++q) {
      const int first = spec->side_cols[2 * q], end = spec->side_cols[2 * q + 1];
      if (spec->number_vp[q] != b.n_vp[q])
        return sfail(h, NZ_ERR_ARG, "player %d: %d victory points drawn, the description has %d", q + 1, spec->number_vp[q], b.n_vp[q]);
      if (first < 0 || end > b.cols || end <= first)
        return sfail(h, NZ_ERR_ARG, "player %d: victory-point columns [%d, %d) on a board of %d", q + 1, first, end, b.cols);
      if ((int64_t)spec->number_vp[q] > (int64_t)b.rows * (end - first))
        return sfail(h, NZ_ERR_ARG, "player %d: %d victory points on a side of %d cells", q + 1, spec->number_vp[q], b.rows * (end - first));
      d.number_vp[q] = spec->number_vp[q];
      d.side_cols[q][0] = first;
      d.side_cols[q][1] = end;
    }
  }
  h->draw = d;
  h->draw_set = true;
  return NZ_OK;
}

// nz_scs_search_set_games with the maps and streams of RandomState(seeds[i]), drawn by scs_draw_kernel.
nz_status nz_scs_search_draw_games(nz_scs_search* h, int64_t n, const uint32_t* seeds_host, void* stream) {
  if (!h || n <= 0 || !seeds_host) return NZ_ERR_ARG;
  if (!h->draw_set) return sfail(h, NZ_ERR_STATE, "no map draw set (nz_scs_search_set_map_draw)");
  if (n < h->n_games) return sfail(h, NZ_ERR_ARG, "%lld games set, the engine plays %d at a time", (long long)n, h->n_games);
  const hipStream_t s = (hipStream_t)stream;
  S_HIP(h, hipSetDevice(h->device));
  S_HIP(h, hipDeviceSynchronize());           // the last plays may still read the rows
  clear_games(h);
  if (!h->rows.ensure((size_t)n, (size_t)h->n_games)) return sfail(h, NZ_ERR_HIP, "device allocation failed (%lld game descriptions)", (long long)n);
  const ScsRules& b = h->host_rules;
  const int64_t T = b.tiles, nv = b.n_vp[0] + b.n_vp[1];
  DrawBufs& d = h->drawn;
  if (!d.ensure((size_t)n, (size_t)T, (size_t)nv)) return sfail(h, NZ_ERR_HIP, "device allocation failed (%lld drawn games)", (long long)n);
  S_HIP(h, hipMemcpyAsync(d.seeds.get(), seeds_host, (size_t)n * 4, hipMemcpyHostToDevice, s));
  S_HIP(h, scs_draw_launch(h->draw, h->made.rules.get(), n, d.seeds.get(), h->rows.rules.get(), h->rows.key.get(),
                           d.terrain.get(), d.vp.get(), d.keys.get(), d.pos.get(), d.err.get(), s));
  // the streams the games go on with: one copy of the states back to the host
  std::vector<uint32_t> keys((size_t)n * 624);
  std::vector<int32_t> pos((size_t)n), err((size_t)n);
  S_HIP(h, hipMemcpyAsync(keys.data(), d.keys.get(), keys.size() * 4, hipMemcpyDeviceToHost, s));
  S_HIP(h, hipMemcpyAsync(pos.data(), d.pos.get(), pos.size() * 4, hipMemcpyDeviceToHost, s));
  S_HIP(h, hipMemcpyAsync(err.data(), d.err.get(), err.size() * 4, hipMemcpyDeviceToHost, s));
  S_HIP(h, hipStreamSynchronize(s));
  for (int64_t i = 0; i < n; ++i) {
    if (err[(size_t)i] == SCS_DRAW_ERR_COST)
      return sfail(h, NZ_ERR_ARG, "game %lld: a terrain with movement cost < 1", (long long)i);
    if (err[(size_t)i] != 0)
      return sfail(h, NZ_ERR_STATE, "game %lld: the map's draws did not settle within the draw kernel's bounds", (long long)i);
  }
  h->game_streams.reserve((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    nz_rng* r = nz_rng_create_state(keys.data() + (size_t)i * 624, pos[(size_t)i], 0, 0.0);
    if (!r) return sfail(h, NZ_ERR_STATE, "game %lld: bad stream position %d", (long long)i, pos[(size_t)i]);
    h->game_streams.push_back(r);
  }
  h->n_drawn = n;
  return use_game_rows(h, n, stream);
}

// Copies of the last nz_scs_search_draw_games (host or device pointers; any may be NULL).
nz_status nz_scs_search_drawn_games(nz_scs_search* h, int64_t* n, float* terrain, int32_t* vp, uint32_t* mt_keys,
                                    int32_t* mt_pos, void* stream) {
  if (!h) return NZ_ERR_ARG;
  if (n) *n = h->n_drawn;
  if (h->n_drawn == 0) return sfail(h, NZ_ERR_STATE, "the games were not drawn by nz_scs_search_draw_games");
  const hipStream_t s = (hipStream_t)stream;
  const size_t N = (size_t)h->n_drawn, T = (size_t)h->host_rules.tiles, nv = (size_t)(h->host_rules.n_vp[0] + h->host_rules.n_vp[1]);
  S_HIP(h, hipSetDevice(h->device));
  if (terrain) S_HIP(h, hipMemcpyAsync(terrain, h->drawn.terrain.get(), N * T * 3 * 4, hipMemcpyDefault, s));
  if (vp) S_HIP(h, hipMemcpyAsync(vp, h->drawn.vp.get(), N * nv * 2 * 4, hipMemcpyDefault, s));
  if (mt_keys) S_HIP(h, hipMemcpyAsync(mt_keys, h->drawn.keys.get(), N * 624 * 4, hipMemcpyDefault, s));
  if (mt_pos) S_HIP(h, hipMemcpyAsync(mt_pos, h->drawn.pos.get(), N * 4, hipMemcpyDefault, s));
  S_HIP(h, hipStreamSynchronize(s));
  return NZ_OK;
}

// HIP-event timing of the persistent kernel on the stream it runs on.  enable >= 0: switch (1 also zeroes the sums).
// out4 (may be NULL): milliseconds summed over launches, launches, v_mfma_f32_16x16x32_bf16 per position, algorithmic
// float32 FLOPs per position.
nz_status nz_scs_search_persist_profile(nz_scs_search* h, int32_t enable, double* out4_host) {
  if (!h) return NZ_ERR_ARG;
  if (enable >= 0) {
    h->persist_profile = enable != 0;
    if (enable) { h->persist_ms = 0.0; h->persist_launches = 0; }
  }
  if (out4_host) {
    out4_host[0] = h->persist_ms; out4_host[1] = (double)h->persist_launches;
    out4_host[2] = (double)h->persist_mfmas; out4_host[3] = (double)h->persist_flops;
  }
  return NZ_OK;
}

// Test hook of the persistent route: keep the leaf evaluations (digest of the planes, post-softmax probabilities, value)
// of `n` games, up to `capacity` each, in the order the game's search consumed them.  n = 0: stop recording.
nz_status nz_scs_search_record(nz_scs_search* h, const int32_t* games_host, int32_t n, int32_t capacity) {
  if (!h || n < 0 || (n > 0 && (!games_host || capacity <= 0))) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  S_HIP(h, hipDeviceSynchronize());
  h->rec = RecordBufs{};
  h->rec.bind(h->pq);
  h->rec_slots = 0;
  if (n == 0) return NZ_OK;
  std::vector<int32_t> slot(h->n_games, -1);
  for (int i = 0; i < n; ++i) {
    if (games_host[i] < 0 || games_host[i] >= h->n_games) return sfail(h, NZ_ERR_ARG, "no game %d", games_host[i]);
    slot[games_host[i]] = i;
  }
  if (!h->rec.ensure(slot.size(), (size_t)n, (size_t)capacity, (size_t)h->p.num_actions))
    return sfail(h, NZ_ERR_HIP, "device allocation failed (recording %d games x %d evaluations)", n, capacity);
  h->rec.bind(h->pq);
  S_HIP(h, hipMemcpy(h->rec.slot.get(), slot.data(), slot.size() * 4, hipMemcpyHostToDevice));
  S_HIP(h, hipMemset(h->pq.rec_count, 0, (size_t)n * 4));
  h->pq.rec_cap = capacity;
  h->rec_slots = n;
  return NZ_OK;
}

// one recorded game: *count evaluations were consumed (those past the capacity are not kept); the arrays take
// min(*count, capacity) rows.  Host pointers; synchronises.
nz_status nz_scs_search_record_read(nz_scs_search* h, int32_t slot, int32_t* count, uint64_t* digests_host, float* probs_host,
                                    float* values_host) {
  if (!h || !count || slot < 0 || slot >= h->rec_slots) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  S_HIP(h, hipDeviceSynchronize());
  S_HIP(h, hipMemcpy(count, h->pq.rec_count + slot, 4, hipMemcpyDeviceToHost));
  const size_t n = (size_t)std::min(*count, h->pq.rec_cap), A = (size_t)h->p.num_actions, at = (size_t)slot * h->pq.rec_cap;
  if (digests_host) S_HIP(h, hipMemcpy(digests_host, h->pq.rec_digest + 2 * at, n * 16, hipMemcpyDeviceToHost));
  if (probs_host) S_HIP(h, hipMemcpy(probs_host, h->pq.rec_probs + at * A, n * A * 4, hipMemcpyDeviceToHost));
  if (values_host) S_HIP(h, hipMemcpy(values_host, h->pq.rec_value + at, n * 4, hipMemcpyDeviceToHost));
  return NZ_OK;
}

// Diagnostic (library built with -DNZ_PERSIST_STAMPS; zeros otherwise): shader ticks of the persistent kernel summed
// over all games and moves since the last reset -- out13: clone, descent, legal mask + list, planes + split, network,
// softmax + value, expansion, backup, whole moves (sum over games), the slowest single (game, move).
nz_status nz_scs_search_persist_ticks(nz_scs_search* h, int64_t* out13_host) {   // (13 values)
  if (!h || !out13_host) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  S_HIP(h, hipDeviceSynchronize());
  int64_t c[16];
  S_HIP(h, hipMemcpy(c, h->p.counters, sizeof(c), hipMemcpyDeviceToHost));
  for (int i = 0; i < 6; ++i) out13_host[i] = c[2 + i];
  for (int i = 6; i < 9; ++i) out13_host[i] = c[5 + i];
  out13_host[9] = c[14];
  for (int i = 0; i < 3; ++i) out13_host[10 + i] = c[8 + i];
  return NZ_OK;
}

// Diagnostic: shader ticks of one per-wavefront-pair network pass (netbench_kernel), `blocks` workgroups of four game
// slots each running `iters` passes; ticks_host[blocks * 4].
nz_status nz_scs_netbench(nz_boardnet* net, int32_t blocks, int32_t iters, uint64_t* ticks_host) {
  if (!net || blocks <= 0 || iters <= 0 || !ticks_host) return NZ_ERR_ARG;
  nz::WaveNet wn{};
  std::string why;
  if (!nz::boardnet_wave_program(net, &wn, &why)) return sfail(nullptr, NZ_ERR_STATE, "%s", why.c_str());
  PersistArgs q{};
  persist_net_args(&q, wn);
  const size_t lds = (size_t)PERSIST_RULES_BYTES + (size_t)PERSIST_GAMES * q.wave_bytes;
  DevBuf<unsigned long long> ticks;
  if (!ticks.ensure((size_t)blocks * PERSIST_GAMES)) return sfail(nullptr, NZ_ERR_HIP, "device allocation failed");
  typedef void (*netbench_fn_t)(PersistArgs, int, unsigned long long*);
  const netbench_fn_t fn = wn.precision == NZ_PREC_BF16 ? (wn.hex ? netbench_kernel<true, PREC_BF16> : netbench_kernel<false, PREC_BF16>)
                                                        : (wn.hex ? netbench_kernel<true> : netbench_kernel<false>);
  hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(PERSIST_THREADS), lds, nullptr, q, iters, ticks.get());
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(ticks_host, ticks.get(), (size_t)blocks * PERSIST_GAMES * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return sfail(nullptr, NZ_ERR_HIP, "netbench: %s", hipGetErrorString(e));
  return NZ_OK;
}

nz_status nz_scs_search_limits(const nz_scs_search* h, int32_t* max_moves, int32_t* max_children) {
  if (!h) return NZ_ERR_ARG;
  if (max_moves) *max_moves = h->p.max_moves;
  if (max_children) *max_children = h->p.maxc;
  return NZ_OK;
}

nz_status nz_scs_search_waves(const nz_scs_search* h, int64_t* waves) {
  if (!h || !waves) return NZ_ERR_ARG;
  *waves = h->waves;
  return NZ_OK;
}

nz_status nz_scs_search_export(nz_scs_search* h, int32_t* actions, int32_t* tree_size, int32_t* n_children,
                               double* bias, double* root_value_sum, int32_t* child_action, int32_t* child_visit,
                               double* child_prior, double* child_value_sum, int64_t* counters_host, void* stream) {
  if (!h) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  const SearchParams& p = h->p;
  return export_records(h, RoundStore{p.rec_action, p.rec_tree_size, p.rec_children, p.rec_child_action, p.rec_child_visit, nullptr, p.rec_bias,
                                      p.rec_root_value_sum, p.rec_child_prior, p.rec_child_value_sum}, (size_t)h->n_games,
                        RoundStore{actions, tree_size, n_children, child_action, child_visit, nullptr, bias, root_value_sum, child_prior, child_value_sum},
                        counters_host, (hipStream_t)stream);
}

}  // extern "C"

// ---- evaluation matches between two agents (nz_scs_match_play) ---------------------------------------------------------
// Tester.Test_using_agents with two MctsAgents that keep their subtrees (Testing/Tester.py:62-118,
// Testing/Agents/Generic/MctsAgent.py:28-39), one match per game slot: two engines hold the same games, each with its
// own trees, search config and network.  Per decision both search the position; the hand-over kernel tells each
// engine's end_move_kernel what to play.
namespace {
struct MatchSide {                 // what the match kernels read of one engine
  const ScsState* real;
  const SNode* nodes;
  const int8_t* half;
  const int32_t* root;
  const int32_t* rec_action;
  const int32_t* error_flag;
  int32_t cap, half_cap;
};
MatchSide match_side(const SearchParams& p) {
  return MatchSide{p.real, p.nodes, p.half, p.root, p.rec_action, p.error_flag, p.cap, p.half_cap};
}

__device__ __forceinline__ bool match_in_step(const ScsState& x, const ScsState& y) {
  return x.length == y.length && x.player == y.player && x.terminal == y.terminal && x.stage == y.stage &&
         x.sub_phase == y.sub_phase && x.terminal_value == y.terminal_value;
}

// max_action (Explorer.py:183-185) of the search that just ended at game g's root: the first maximum of the children's
// visits, as end_move_kernel picks it; -1 for a root without children (end_move_kernel reports that)
__device__ __forceinline__ int match_root_choice(const MatchSide& s, int g) {
  const SNode* nodes = s.nodes + (size_t)g * s.cap + (size_t)s.half[g] * s.half_cap;
  const SNode root = nodes[s.root[g]];
  if (root.n_children == 0) return -1;
  int best = 0;
  for (int j = 1; j < root.n_children; ++j)
    if (nodes[root.child_base + j].visit > nodes[root.child_base + best].visit) best = j;
  return nodes[root.child_base + best].action;
}

// out3 (zeroed by the host): matches still being played, and the two engines' error flags; bit 64 of the first flag:
// the engines no longer hold the same game
__global__ void match_live_kernel(MatchSide a, MatchSide b, int n, int32_t* __restrict__ out3) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = g < n;
  const bool live = in && !a.real[g].terminal;
  const bool apart = in && !match_in_step(a.real[g], b.real[g]);
  const int n_live = __popcll(__ballot(live));
  const bool any_apart = __ballot(apart) != 0;
  if ((threadIdx.x & 63) == 0) {
    if (n_live) atomicAdd(&out3[0], n_live);
    if (any_apart) atomicOr(&out3[1], 64);
  }
  if (g == 0) {
    atomicOr(&out3[1], *a.error_flag);
    atomicOr(&out3[2], *b.error_flag);
  }
}

// The hand-over of one decision, after both searches: the player to move differs from match to match (SCS turns have
// phases), so per match the mover's engine gets -1 ("choose yourself": its end_move_kernel takes max_action) and the
// opponent's engine gets the action the mover will take -- read from the mover's root exactly as end_move_kernel reads
// it, because one end_move launch per engine serves movers and followers alike (match_tally_kernel holds the two
// engines' records against each other).  Agent 1 moves for player index 1 (oracle/agents.py play_match).  The action
// also enters the match record [n][max_moves].
__global__ void match_handover_kernel(MatchSide a, MatchSide b, int n, int max_moves, int32_t* __restrict__ forced_a,
                                      int32_t* __restrict__ forced_b, int32_t* __restrict__ actions) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  forced_a[g] = -1;
  forced_b[g] = -1;
  const ScsState& st = a.real[g];
  if (st.terminal) return;
  const int move = st.length;
  if (move >= max_moves) return;                         // (end_move_kernel reports it)
  const bool a_moves = st.player == 1;
  const int action = a_moves ? match_root_choice(a, g) : match_root_choice(b, g);
  if (action < 0) return;
  (a_moves ? forced_b : forced_a)[g] = action;
  actions[(size_t)g * max_moves + move] = action;
}

// tally [8] (zeroed by the host): matches, wins of player 1 (terminal value +1), wins of player 2 (-1), draws,
// unfinished (stopped at max_moves), sum and maximum of the match lengths, and the matches in which the two engines'
// records or the match record disagree or the record has a gap (a result with any of those is refused).  A round on one
// engine (nz_scs_agent_match_play) has no second side: b.real is null and `actions` is a's own record.
__global__ void match_tally_kernel(MatchSide a, MatchSide b, int n, int max_moves, const int32_t* __restrict__ actions,
                                   unsigned long long* __restrict__ tally) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = g < n;
  int length = 0, value = 0;
  bool done = false, bad = false;
  if (in) {
    const ScsState& st = a.real[g];
    length = st.length;
    value = st.terminal_value;
    done = st.terminal != 0;
    const bool two = b.real != nullptr;
    bad = (two && !match_in_step(st, b.real[g])) || length > max_moves;
    for (int m = 0; m < length && !bad; ++m) {
      const size_t at = (size_t)g * max_moves + m;
      bad = actions[at] < 0 || (two && (a.rec_action[at] != actions[at] || b.rec_action[at] != actions[at]));
    }
  }
  const int n_in = __popcll(__ballot(in)), n_p1 = __popcll(__ballot(in && done && value > 0)),
            n_p2 = __popcll(__ballot(in && done && value < 0)), n_draw = __popcll(__ballot(in && done && value == 0)),
            n_open = __popcll(__ballot(in && !done));
  if ((threadIdx.x & 63) == 0) {               // one vector atomic per wavefront and category
    if (n_in) atomicAdd(&tally[0], (unsigned long long)n_in);
    if (n_p1) atomicAdd(&tally[1], (unsigned long long)n_p1);
    if (n_p2) atomicAdd(&tally[2], (unsigned long long)n_p2);
    if (n_draw) atomicAdd(&tally[3], (unsigned long long)n_draw);
    if (n_open) atomicAdd(&tally[4], (unsigned long long)n_open);
  }
  if (in) {
    atomicAdd(&tally[5], (unsigned long long)length);
    atomicMax(&tally[6], (unsigned long long)length);
    if (bad) atomicAdd(&tally[7], 1ull);
  }
}

// The tally of h's round against `record` (with `other` the second engine's side, or none), read out into out_host, and
// the record copied to actions_dev; either may be null.  Refused matches fail with `refused` (one %lld: how many).
nz_status tally_result(nz_scs_search* h, int64_t* tally, const MatchSide& other, const int32_t* record, const char* refused,
                       nz_scs_match_tally* out_host, int32_t* actions_dev, hipStream_t s) {
  const int G = h->n_games, MAX_MOVES = h->p.max_moves;
  S_HIP(h, hipMemsetAsync(tally, 0, 8 * sizeof(int64_t), s));
  hipLaunchKernelGGL(match_tally_kernel, dim3((G + 127) / 128), dim3(128), 0, s, match_side(h->p), other, G, MAX_MOVES, record,
                     (unsigned long long*)tally);
  S_HIP(h, hipGetLastError());
  int64_t t[8];
  S_HIP(h, hipMemcpyAsync(t, tally, sizeof(t), hipMemcpyDeviceToHost, s));
  if (actions_dev)
    S_HIP(h, hipMemcpyAsync(actions_dev, record, (size_t)G * MAX_MOVES * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  S_HIP(h, hipStreamSynchronize(s));
  if (t[7] != 0) return sfail(h, NZ_ERR_STATE, refused, (long long)t[7]);
  if (out_host) {
    out_host->matches = t[0]; out_host->p1_wins = t[1]; out_host->p2_wins = t[2]; out_host->draws = t[3];
    out_host->unfinished = t[4]; out_host->length_sum = t[5]; out_host->length_max = t[6];
  }
  return NZ_OK;
}
}  // namespace

extern "C" nz_status nz_scs_match_play(nz_scs_search* a1, nz_boardnet* net1, nz_scs_search* a2, nz_boardnet* net2,
                                       int32_t max_moves, void* stream) {
  return nz_scs_match_play_from(a1, net1, a2, net2, nullptr, max_moves, stream);
}

// nz_scs_match_play with every match started at its opening (scs_openings.hip), the same one in both engines.
extern "C" nz_status nz_scs_match_play_from(nz_scs_search* a1, nz_boardnet* net1, nz_scs_search* a2, nz_boardnet* net2,
                                            const nz_scs_openings* openings, int32_t max_moves, void* stream) {
  if (!a1 || !a2 || !net1 || !net2) return sfail(a1, NZ_ERR_ARG, "null argument");
  if (a1 == a2) return sfail(a1, NZ_ERR_ARG, "a match needs two engines: each agent keeps its own trees");
  a1->match_peer = nullptr;
  if (a1->cfg.training || a2->cfg.training) return sfail(a1, NZ_ERR_ARG, "evaluation agents are training = 0 engines (MctsAgent.py:14-20)");
  if (a1->n_games != a2->n_games || a1->device != a2->device)
    return sfail(a1, NZ_ERR_ARG, "the two engines hold %d and %d games on devices %d and %d", a1->n_games, a2->n_games, a1->device, a2->device);
  if (memcmp(&a1->host_rules, &a2->host_rules, sizeof(ScsRules)) != 0)
    return sfail(a1, NZ_ERR_ARG, "the two engines were created with different game descriptions");
  if (!openings_ok(a1, openings)) return NZ_ERR_ARG;      // (refused before anything is reset; a2 has a1's description)
  S_HIP(a1, hipSetDevice(a1->device));
  hipStream_t s1 = (hipStream_t)stream;
  const int G = a1->n_games, MAX_MOVES = a1->p.max_moves;
  if (a1->n_game_rows != a2->n_game_rows)
    return sfail(a1, NZ_ERR_ARG, "per-game maps: %lld set on agent 1, %lld on agent 2", (long long)a1->n_game_rows, (long long)a2->n_game_rows);
  // agent 2's failures are reported on agent 1's handle, the one the caller asks
  auto on2 = [&](nz_status st) {
    if (st != NZ_OK) a1->error = "agent 2: " + a2->error;
    return st;
  };
  if (a1->n_game_rows > 0) {                  // every match on its own map: the same one in both engines
    if (a1->n_game_rows < G) return sfail(a1, NZ_ERR_ARG, "%d matches, %lld maps set", G, (long long)a1->n_game_rows);
    std::vector<uint64_t> k1((size_t)G * 2), k2((size_t)G * 2);
    S_HIP(a1, hipStreamSynchronize(s1));
    S_HIP(a1, hipMemcpy(k1.data(), a1->rows.key.get(), k1.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    S_HIP(a1, hipMemcpy(k2.data(), a2->rows.key.get(), k2.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (int g = 0; g < G; ++g)
      if (k1[(size_t)g * 2] != k2[(size_t)g * 2] || k1[(size_t)g * 2 + 1] != k2[(size_t)g * 2 + 1])
        return sfail(a1, NZ_ERR_ARG, "match %d: the two engines hold different maps (digests %016llx%016llx and %016llx%016llx)", g,
                     (unsigned long long)k1[(size_t)g * 2], (unsigned long long)k1[(size_t)g * 2 + 1],
                     (unsigned long long)k2[(size_t)g * 2], (unsigned long long)k2[(size_t)g * 2 + 1]);
    if (nz_status st = slots_read_own_rows(a1)) return st;
    if (nz_status st = on2(slots_read_own_rows(a2))) return st;
  }
  PlayRoute r1, r2;
  if (nz_status st = play_prepare(a1, net1, &r1, stream)) return st;
  if (nz_status st = on2(play_prepare(a2, net2, &r2, stream))) return st;
  if (r1.persist && r2.persist && a1->persist_fn == a2->persist_fn && r1.persist_lds != r2.persist_lds)
    // one kernel, two networks: the attribute is the kernel's, so it must cover the larger of the two launches
    S_HIP(a1, hipFuncSetAttribute((const void*)a1->persist_fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)std::max(r1.persist_lds, r2.persist_lds)));
  MatchBufs& m = a1->match;
  if (!m.ensure((size_t)G, (size_t)MAX_MOVES)) return sfail(a1, NZ_ERR_HIP, "allocation failed (match buffers, stream, events)");
  // The two searches of a decision are independent: agent 2's runs on a stream of its own between a fork and a join
  // event.  One stream when the agents share a network object (the wave-by-wave route evaluates in the network's own
  // buffers) or for the A/B measurement (NZ_SCS_MATCH_STREAMS=1, scripts/time_scs_match.py).
  const char* env_streams = getenv("NZ_SCS_MATCH_STREAMS");
  const bool two_streams = net1 != net2 && !(env_streams && atoi(env_streams) == 1);
  hipStream_t s2 = two_streams ? m.stream.get() : s1;
  int32_t* const forced1 = m.forced.get();
  int32_t* const forced2 = m.forced.get() + G;
  if (nz_status st = nz_scs_search_reset_to(a1, openings, stream)) {
    (void)nz_scs_search_reset(a2, stream);                // a refused opening leaves both engines at the start
    return st;
  }
  if (nz_status st = on2(nz_scs_search_reset_to(a2, openings, stream))) return st;
  S_HIP(a1, hipMemsetAsync(m.actions.get(), 0xFF, (size_t)G * MAX_MOVES * sizeof(int32_t), s1));    // -1: not played
  if (openings && openings->max_plies > 0)     // the opening's plies at their decision numbers: all a fresh engine's record holds
    S_HIP(a1, hipMemcpyAsync(m.actions.get(), a1->p.rec_action, (size_t)G * MAX_MOVES * sizeof(int32_t), hipMemcpyDeviceToDevice, s1));
  a1->waves = a2->waves = 0;
  a1->round_games = a2->round_games = 0;
  const MatchSide m1 = match_side(a1->p), m2 = match_side(a2->p);
  const dim3 grid1((G + 127) / 128), block1(128);
  const int move_limit = max_moves > 0 && max_moves < MAX_MOVES ? max_moves : MAX_MOVES;
  auto state_check = [&](int32_t* live) -> nz_status {   // the decision's one wait: live matches and both engines' flags
    S_HIP(a1, hipMemsetAsync(m.state.get(), 0, 3 * sizeof(int32_t), s1));
    hipLaunchKernelGGL(match_live_kernel, grid1, block1, 0, s1, m1, m2, G, m.state.get());
    S_HIP(a1, hipMemcpyAsync(m.pinned.get(), m.state.get(), 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s1));
    S_HIP(a1, hipStreamSynchronize(s1));
    const int32_t f1 = m.pinned[1], f2 = m.pinned[2];
    if (f1 & 64) return sfail(a1, NZ_ERR_STATE, "internal: the two engines no longer hold the same games");
    if (f1 || f2)
      return sfail(a1, NZ_ERR_OVERFLOW, "device check failed (agent 1 flag %d, agent 2 flag %d: %s%s)", f1, f2, FLAG_TEXT,
                   (f1 & 128 ? dead_end_text(a1, f1, s1) : dead_end_text(a2, f2, s1)).c_str());
    *live = m.pinned[0];
    return NZ_OK;
  };
  nz_status st = NZ_OK;
  for (int move = 0; move < move_limit; ++move) {
    int32_t live = 0;
    if ((st = state_check(&live)) != NZ_OK) return st;
    if (live == 0) break;
    if (two_streams) {
      S_HIP(a1, hipEventRecord(m.ev_fork.get(), s1));
      S_HIP(a1, hipStreamWaitEvent(s2, m.ev_fork.get(), 0));
    }
    // a persistent search is one launch; a wave-by-wave one keeps the host until its last wave: enqueue the former first
    if (!r1.persist && r2.persist) {
      st = on2(search_move(a2, net2, r2, s2));
      if (st == NZ_OK) st = search_move(a1, net1, r1, s1);
    } else {
      st = search_move(a1, net1, r1, s1);
      if (st == NZ_OK) st = on2(search_move(a2, net2, r2, s2));
    }
    if (st != NZ_OK) {
      if (two_streams) (void)hipStreamSynchronize(s2);
      return st;
    }
    if (two_streams) {
      S_HIP(a1, hipEventRecord(m.ev_join.get(), s2));
      S_HIP(a1, hipStreamWaitEvent(s1, m.ev_join.get(), 0));
    }
    hipLaunchKernelGGL(match_handover_kernel, grid1, block1, 0, s1, m1, m2, G, MAX_MOVES, forced1, forced2, m.actions.get());
    const dim3 grid_end((G + 63) / 64), block_end(64);
    hipLaunchKernelGGL(end_move_kernel, grid_end, block_end, 0, s1, a1->p, (const double*)nullptr, (const int32_t*)forced1);
    hipLaunchKernelGGL(compact_kernel, dim3(G), dim3(64), 0, s1, a1->p);
    hipLaunchKernelGGL(end_move_kernel, grid_end, block_end, 0, s1, a2->p, (const double*)nullptr, (const int32_t*)forced2);
    hipLaunchKernelGGL(compact_kernel, dim3(G), dim3(64), 0, s1, a2->p);
    S_HIP(a1, hipGetLastError());
  }
  rest_counters(a1);
  rest_counters(a2);
  int32_t live = 0;
  if ((st = state_check(&live)) != NZ_OK) return st;     // (the last decision's flags)
  a1->match_peer = a2;
  return NZ_OK;
}

extern "C" nz_status nz_scs_match_result(nz_scs_search* a1, nz_scs_search* a2, nz_scs_match_tally* out_host,
                                         int32_t* actions_dev, void* stream) {
  if (!a1 || !a2) return sfail(a1, NZ_ERR_ARG, "null argument");
  if (a1->match_peer != a2) return sfail(a1, NZ_ERR_STATE, "no match round was played on these two handles");
  S_HIP(a1, hipSetDevice(a1->device));
  return tally_result(a1, a1->match.tally.get(), match_side(a2->p), a1->match.actions.get(),
                      "internal: in %lld matches the two engines' records and the match record disagree", out_host, actions_dev,
                      (hipStream_t)stream);
}

// ---- evaluation matches against scripted agents (nz_scs_agent_match_play) ----------------------------------------------
// Tester.Test_using_agents where at most one side is an MctsAgent: the other sides are the bare policy or a random mover
// (scs_agents.hip).  `h` holds the games; its own search is the MCTS side, which searches on every ply (the mover's
// choose_action, the opponent's update_subtree) and takes the scripted mover's action through end_move_kernel's forced
// actions.  Without an MCTS side no simulation runs: the agents' kernel steps the games itself and the handle's trees
// stay the unexpanded roots of its reset.
namespace {
void agent_args(nz_scs_search* h, AgentArgs* a) {
  AgentBufs& b = h->agents;
  const ScsRules& R = h->host_rules;
  a->rules = h->p.rules; a->rules_row = h->p.rules_row; a->real = h->p.real;
  a->n_games = h->n_games; a->max_moves = h->p.max_moves; a->num_actions = R.planes * R.tiles;
  a->forced = b.forced.get(); a->rec_action = h->p.rec_action; a->slot = b.slot.get(); a->digest = b.digest.get(); a->err = b.err.get();
  for (int i = 0; i < 2; ++i) b.side[i].bind(a->side[i]);
}
}  // namespace

extern "C" nz_status nz_scs_agent_match_play(nz_scs_search* h, const nz_scs_agent* p1, const nz_scs_agent* p2, int32_t max_moves,
                                             void* stream) {
  return nz_scs_agent_match_play_from(h, p1, p2, nullptr, max_moves, stream);
}

// nz_scs_agent_match_play with every match started at its opening (scs_openings.hip).
extern "C" nz_status nz_scs_agent_match_play_from(nz_scs_search* h, const nz_scs_agent* p1, const nz_scs_agent* p2,
                                                  const nz_scs_openings* openings, int32_t max_moves, void* stream) {
  if (!h || !p1 || !p2) return sfail(h, NZ_ERR_ARG, "null argument");
  if (!openings_ok(h, openings)) return NZ_ERR_ARG;       // (refused before anything is reset)
  const nz_scs_agent* const ag[2] = {p1, p2};
  h->agents.kinds[0] = h->agents.kinds[1] = -1;
  int mcts = -1;
  for (int i = 0; i < 2; ++i) {
    const int kind = ag[i]->kind;
    if (kind != NZ_AGENT_MCTS && kind != NZ_AGENT_POLICY && kind != NZ_AGENT_RANDOM) return sfail(h, NZ_ERR_ARG, "agent %d: unknown kind %d", i + 1, kind);
    if (kind != NZ_AGENT_RANDOM && !ag[i]->net) return sfail(h, NZ_ERR_ARG, "agent %d: a policy or MCTS agent needs a network", i + 1);
    if (kind == NZ_AGENT_RANDOM && !ag[i]->seeds_host) return sfail(h, NZ_ERR_ARG, "agent %d: a random agent needs one seed per match", i + 1);
    if (kind == NZ_AGENT_MCTS) {
      if (mcts >= 0)
        return sfail(h, NZ_ERR_ARG, "both agents are MCTS agents: each needs a handle of its own, use nz_scs_match_play");
      mcts = i;
    }
  }
  if (mcts >= 0 && h->cfg.training) return sfail(h, NZ_ERR_ARG, "evaluation agents are training = 0 engines (MctsAgent.py:14-20)");
  if (mcts >= 0 && !h->cfg.keep_subtree) return sfail(h, NZ_ERR_ARG, "the MCTS agent keeps its subtree (keep_subtree = 1)");
  S_HIP(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const int G = h->n_games, MAX_MOVES = h->p.max_moves;
  const ScsRules& R = h->host_rules;
  const size_t A = (size_t)R.planes * R.tiles, GM = (size_t)G * MAX_MOVES;
  if (h->n_game_rows > 0) {                    // every match on its own map
    if (h->n_game_rows < G) return sfail(h, NZ_ERR_ARG, "%d matches, %lld maps set", G, (long long)h->n_game_rows);
    S_HIP(h, hipStreamSynchronize(s));
    if (nz_status st = slots_read_own_rows(h)) return st;
  }
  AgentBufs& b = h->agents;
  const int kinds[2] = {p1->kind, p2->kind};
  if (!b.ensure(kinds, (size_t)G, (size_t)MAX_MOVES, A)) return sfail(h, NZ_ERR_HIP, "allocation failed (agent buffers)");
  PlayRoute route;
  if (mcts >= 0) {
    if (nz_status st = play_prepare(h, ag[mcts]->net, &route, stream)) return st;
  } else {
    h->persist_used = 0;
  }
  AgentArgs a{};
  agent_args(h, &a);
  a.step = mcts < 0 ? 1 : 0;
  for (int i = 0; i < 2; ++i) {
    AgentSide& sd = a.side[i];
    sd.kind = ag[i]->kind;
    if (sd.kind == NZ_AGENT_POLICY)            // the network fits the game and holds every match's position
      if (nz_status st = net_fits(h, ag[i]->net, i + 1, &sd.net_rows, &sd.row_stride)) return st;
  }
  if (nz_status st = nz_scs_search_reset_to(h, openings, stream)) return st;
  h->waves = 0;
  h->round_games = 0;
  h->match_peer = nullptr;
  // the scripted sides' streams (rebuilt from the seeds every round) and records
  for (int i = 0; i < 2; ++i) {
    AgentSideBufs& sb = b.side[i];
    if (ag[i]->kind == NZ_AGENT_MCTS) continue;
    if (ag[i]->kind == NZ_AGENT_RANDOM) {
      S_HIP(h, hipMemcpyAsync(sb.seeds.get(), ag[i]->seeds_host, (size_t)G * sizeof(uint32_t), hipMemcpyHostToDevice, s));
      S_HIP(h, agent_seed_launch(sb.seeds.get(), sb.mt_keys.get(), sb.mt_pos.get(), G, s));
    }
    S_HIP(h, hipMemsetAsync(sb.rec_action.get(), 0xFF, GM * sizeof(int32_t), s));     // -1: not this side's decision
    S_HIP(h, hipMemsetAsync(sb.rec_n_legal.get(), 0, GM * sizeof(int32_t), s));
    S_HIP(h, hipMemsetAsync(sb.rec_prob.get(), 0, GM * sizeof(float), s));
    if (sb.hook_slots > 0) S_HIP(h, hipMemsetAsync(sb.hook_count.get(), 0, (size_t)sb.hook_slots * sizeof(int32_t), s));
  }
  S_HIP(h, hipMemsetAsync(b.err.get(), 0, (size_t)G * sizeof(int32_t), s));
  S_HIP(h, hipStreamSynchronize(s));           // (the seeds are the caller's memory)
  const int move_limit = max_moves > 0 && max_moves < MAX_MOVES ? max_moves : MAX_MOVES;
  auto state_check = [&](int32_t* live) -> nz_status {   // the decision's one wait: live matches, the engine's flag, the agents' error words
    S_HIP(h, hipMemsetAsync(b.state.get(), 0, 3 * sizeof(int32_t), s));
    S_HIP(h, agent_live_launch(h->p.real, G, h->p.error_flag, b.err.get(), b.state.get(), s));
    S_HIP(h, hipMemcpyAsync(b.pinned.get(), b.state.get(), 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    S_HIP(h, hipStreamSynchronize(s));
    if (b.pinned[1])
      return sfail(h, NZ_ERR_OVERFLOW, "device check failed (flag %d: %s%s)", b.pinned[1], FLAG_TEXT, dead_end_text(h, b.pinned[1], s).c_str());
    if (b.pinned[2])
      return sfail(h, NZ_ERR_OVERFLOW, "scripted agent check failed (flags %d: 1 randint rejection cap, 2 no legal action, "
                   "4 game longer than the bound computed at create)", b.pinned[2]);
    *live = b.pinned[0];
    return NZ_OK;
  };
  nz_status st = NZ_OK;
  for (int move = 0; move < move_limit; ++move) {
    int32_t live = 0;
    if ((st = state_check(&live)) != NZ_OK) return st;
    if (live == 0) break;
    if (mcts >= 0 && (st = search_move(h, ag[mcts]->net, route, s)) != NZ_OK) return st;
    // The positions a policy agent decides go straight into its network's input rows; the count stays on the device.
    // Side by side on the one stream: two policy agents may share a network, whose input rows hold one side's
    // positions at a time (the evaluations land in the side's own probs / value).
    for (int i = 0; i < 2; ++i) {
      if (ag[i]->kind != NZ_AGENT_POLICY) continue;
      S_HIP(h, hipMemsetAsync(b.side[i].count.get(), 0, sizeof(int32_t), s));
      S_HIP(h, agent_image_launch(a, i, s));
      if (nz_boardnet_forward_rows(ag[i]->net, G, b.side[i].count.get(), nullptr, b.side[i].probs.get(), b.side[i].value.get(), stream) != NZ_OK)
        return sfail(h, NZ_ERR_HIP, "agent %d's network: %s", i + 1, nz_boardnet_last_error(ag[i]->net));
    }
    S_HIP(h, agent_act_launch(a, s));
    if (mcts >= 0) {
      hipLaunchKernelGGL(end_move_kernel, dim3((G + 63) / 64), dim3(64), 0, s, h->p, (const double*)nullptr, (const int32_t*)b.forced.get());
      hipLaunchKernelGGL(compact_kernel, dim3(G), dim3(64), 0, s, h->p);
      S_HIP(h, hipGetLastError());
    }
  }
  rest_counters(h);
  int32_t live = 0;
  if ((st = state_check(&live)) != NZ_OK) return st;     // (the last decision's flags)
  b.kinds[0] = p1->kind;
  b.kinds[1] = p2->kind;
  return NZ_OK;
}

extern "C" nz_status nz_scs_agent_match_result(nz_scs_search* h, nz_scs_match_tally* out_host, int32_t* actions_dev, void* stream) {
  if (!h) return sfail(h, NZ_ERR_ARG, "null argument");
  if (h->agents.kinds[0] < 0) return sfail(h, NZ_ERR_STATE, "no agent match round was played on this handle");
  S_HIP(h, hipSetDevice(h->device));
  return tally_result(h, h->agents.tally.get(), MatchSide{}, h->p.rec_action, "internal: the action record of %lld matches has a gap",
                      out_host, actions_dev, (hipStream_t)stream);
}

extern "C" nz_status nz_scs_agent_match_decisions(nz_scs_search* h, int32_t side, int32_t* actions_dev, int32_t* n_legal_dev,
                                                  float* probs_dev, void* stream) {
  if (!h || side < 0 || side > 1) return sfail(h, NZ_ERR_ARG, "bad argument");
  if (h->agents.kinds[0] < 0) return sfail(h, NZ_ERR_STATE, "no agent match round was played on this handle");
  if (h->agents.kinds[side] == NZ_AGENT_MCTS) return sfail(h, NZ_ERR_ARG, "agent %d is the MCTS agent: read it with nz_scs_search_export", side + 1);
  S_HIP(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const AgentSideBufs& sb = h->agents.side[side];
  const size_t GM = (size_t)h->n_games * h->p.max_moves;
  if (actions_dev) S_HIP(h, hipMemcpyAsync(actions_dev, sb.rec_action.get(), GM * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (n_legal_dev) S_HIP(h, hipMemcpyAsync(n_legal_dev, sb.rec_n_legal.get(), GM * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (probs_dev) S_HIP(h, hipMemcpyAsync(probs_dev, sb.rec_prob.get(), GM * sizeof(float), hipMemcpyDeviceToDevice, s));
  return NZ_OK;
}

// Test hook: keep the policy agent's evaluations (digest of the planes, post-softmax probabilities, value) of `n` matches,
// up to `capacity` each, in the order the agent consumed them.  n = 0: stop recording.
extern "C" nz_status nz_scs_agent_record(nz_scs_search* h, int32_t side, const int32_t* games_host, int32_t n, int32_t capacity) {
  if (!h || side < 0 || side > 1 || n < 0 || (n > 0 && (!games_host || capacity <= 0))) return sfail(h, NZ_ERR_ARG, "bad argument");
  S_HIP(h, hipSetDevice(h->device));
  S_HIP(h, hipDeviceSynchronize());
  AgentSideBufs& sb = h->agents.side[side];
  sb.hook_slots = sb.hook_cap = 0;
  sb.hook_slot.reset(); sb.hook_count.reset(); sb.hook_digest.reset(); sb.hook_probs.reset(); sb.hook_value.reset();
  if (n == 0) return NZ_OK;
  std::vector<int32_t> slot(h->n_games, -1);
  for (int i = 0; i < n; ++i) {
    if (games_host[i] < 0 || games_host[i] >= h->n_games) return sfail(h, NZ_ERR_ARG, "no match %d", games_host[i]);
    slot[games_host[i]] = i;
  }
  const size_t N = (size_t)n * capacity, A = (size_t)h->p.num_actions;
  if (!(sb.hook_slot.ensure(slot.size()) && sb.hook_count.ensure(n) && sb.hook_digest.ensure(N * 2) && sb.hook_probs.ensure(N * A) &&
        sb.hook_value.ensure(N))) {
    sb.hook_slot.reset(); sb.hook_count.reset(); sb.hook_digest.reset(); sb.hook_probs.reset(); sb.hook_value.reset();
    return sfail(h, NZ_ERR_HIP, "device allocation failed (recording %d matches x %d evaluations)", n, capacity);
  }
  S_HIP(h, hipMemcpy(sb.hook_slot.get(), slot.data(), slot.size() * 4, hipMemcpyHostToDevice));
  S_HIP(h, hipMemset(sb.hook_count.get(), 0, (size_t)n * 4));
  sb.hook_slots = n;
  sb.hook_cap = capacity;
  return NZ_OK;
}

extern "C" nz_status nz_scs_agent_record_read(nz_scs_search* h, int32_t side, int32_t slot, int32_t* count, uint64_t* digests_host,
                                              float* probs_host, float* values_host) {
  if (!h || side < 0 || side > 1 || !count || slot < 0 || slot >= h->agents.side[side].hook_slots) return sfail(h, NZ_ERR_ARG, "bad argument");
  S_HIP(h, hipSetDevice(h->device));
  S_HIP(h, hipDeviceSynchronize());
  const AgentSideBufs& sb = h->agents.side[side];
  S_HIP(h, hipMemcpy(count, sb.hook_count.get() + slot, 4, hipMemcpyDeviceToHost));
  const size_t n = (size_t)std::min(*count, sb.hook_cap), A = (size_t)h->p.num_actions, at = (size_t)slot * sb.hook_cap;
  if (digests_host) S_HIP(h, hipMemcpy(digests_host, sb.hook_digest.get() + 2 * at, n * 16, hipMemcpyDeviceToHost));
  if (probs_host) S_HIP(h, hipMemcpy(probs_host, sb.hook_probs.get() + at * A, n * A * 4, hipMemcpyDeviceToHost));
  if (values_host) S_HIP(h, hipMemcpy(values_host, sb.hook_value.get() + at, n * 4, hipMemcpyDeviceToHost));
  return NZ_OK;
}

// ---- matches from opening positions (scs_openings.hip) -----------------------------------------------------------------
// The host side of the three opening kernels: the checks that need no launch, the copies, and the error words read back.
extern "C" nz_status nz_scs_search_reset_to(nz_scs_search* h, const nz_scs_openings* o, void* stream) {
  if (!h) return NZ_ERR_ARG;
  if (!o || o->max_plies == 0) return nz_scs_search_reset(h, stream);
  if (!openings_ok(h, o)) return NZ_ERR_ARG;
  S_HIP(h, hipSetDevice(h->device));
  const hipStream_t s = (hipStream_t)stream;
  const int G = h->n_games, P = o->max_plies;
  OpeningBufs& b = h->openings;
  if (!(b.actions.ensure((size_t)G * P) && b.n_plies.ensure(G) && b.err.ensure(G)))
    return sfail(h, NZ_ERR_HIP, "device allocation failed (openings)");
  std::vector<int32_t> np(G, P), err(G, 0);
  if (o->n_plies) std::copy(o->n_plies, o->n_plies + G, np.begin());
  S_HIP(h, hipMemcpyAsync(b.actions.get(), o->actions, (size_t)G * P * sizeof(int32_t), hipMemcpyHostToDevice, s));
  S_HIP(h, hipMemcpyAsync(b.n_plies.get(), np.data(), (size_t)G * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (nz_status st = nz_scs_search_reset(h, stream)) return st;
  S_HIP(h, opening_apply_launch(opening_games(h), G, b.actions.get(), b.n_plies.get(), P, h->p.real, h->p.rec_action, h->p.max_moves,
                                b.err.get(), s));
  S_HIP(h, hipMemcpyAsync(err.data(), b.err.get(), (size_t)G * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  S_HIP(h, hipStreamSynchronize(s));             // (the openings are the caller's memory; the error words decide the status)
  for (int g = 0; g < G; ++g) {
    if (!err[g]) continue;
    if (nz_status st = nz_scs_search_reset(h, stream)) return st;      // nothing of a refused call survives
    S_HIP(h, hipStreamSynchronize(s));
    const int ply = opening_err_ply(err[g]);
    return sfail(h, NZ_ERR_ARG, "match %d, ply %d: action %d: %s", g, ply, ply < np[g] ? o->actions[(size_t)g * P + ply] : -1,
                 opening_reason(err[g]));
  }
  return NZ_OK;
}

extern "C" nz_status nz_scs_openings_draw(nz_scs_search* h, const uint32_t* seeds_host, int32_t plies, int32_t* actions_out,
                                          int32_t* n_plies_out, void* stream) {
  if (!h || !seeds_host || !actions_out || !n_plies_out) return sfail(h, NZ_ERR_ARG, "null argument");
  if (plies < 1 || plies > h->p.max_moves) return sfail(h, NZ_ERR_ARG, "openings of %d plies: 1 .. %d", plies, h->p.max_moves);
  S_HIP(h, hipSetDevice(h->device));
  const hipStream_t s = (hipStream_t)stream;
  const int G = h->n_games;
  if (h->n_game_rows > 0) {                      // every match on its own map, as the match calls set it
    if (h->n_game_rows < G) return sfail(h, NZ_ERR_ARG, "%d matches, %lld maps set", G, (long long)h->n_game_rows);
    S_HIP(h, hipStreamSynchronize(s));
    if (nz_status st = slots_read_own_rows(h)) return st;
  }
  OpeningBufs& b = h->openings;
  if (!(b.seeds.ensure(G) && b.actions.ensure((size_t)G * plies) && b.n_plies.ensure(G) && b.err.ensure(G)))
    return sfail(h, NZ_ERR_HIP, "device allocation failed (openings)");
  std::vector<int32_t> err(G, 0);
  S_HIP(h, hipMemcpyAsync(b.seeds.get(), seeds_host, (size_t)G * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  S_HIP(h, opening_draw_launch(opening_games(h), G, b.seeds.get(), plies, b.actions.get(), b.n_plies.get(), b.err.get(), s));
  S_HIP(h, hipMemcpyAsync(actions_out, b.actions.get(), (size_t)G * plies * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  S_HIP(h, hipMemcpyAsync(n_plies_out, b.n_plies.get(), (size_t)G * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  S_HIP(h, hipMemcpyAsync(err.data(), b.err.get(), (size_t)G * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  S_HIP(h, hipStreamSynchronize(s));
  for (int g = 0; g < G; ++g)
    if (err[g]) return sfail(h, NZ_ERR_OVERFLOW, "match %d, ply %d: %s", g, opening_err_ply(err[g]), opening_reason(err[g]));
  return NZ_OK;
}

extern "C" nz_status nz_scs_openings_expand(nz_scs_search* h, const int32_t* frontier_host, int32_t n, int32_t depth,
                                            int32_t* counts_host, int32_t* children_host, uint64_t* keys_host, void* stream) {
  if (!h || n <= 0 || depth < 0 || !counts_host || (depth > 0 && !frontier_host) || ((children_host == nullptr) != (keys_host == nullptr)))
    return sfail(h, NZ_ERR_ARG, "bad argument");
  if (depth >= h->p.max_moves) return sfail(h, NZ_ERR_ARG, "prefixes of %d plies: 0 .. %d", depth, h->p.max_moves - 1);
  if (h->n_game_rows > 0)
    return sfail(h, NZ_ERR_STATE, "per-game maps are set: one frontier belongs to one map (draw openings per match instead)");
  const int A = h->p.num_actions;
  for (int f = 0; f < n; ++f)
    for (int ply = 0; ply < depth; ++ply) {
      const int a = frontier_host[(size_t)f * depth + ply];
      if (a < 0 || a >= A) return sfail(h, NZ_ERR_ARG, "prefix %d, ply %d: action %d outside 0 .. %d", f, ply, a, A - 1);
    }
  S_HIP(h, hipSetDevice(h->device));
  const hipStream_t s = (hipStream_t)stream;
  OpeningBufs& b = h->openings;
  if (!(b.actions.ensure(std::max<size_t>(1, (size_t)n * depth)) && b.counts.ensure(n) && b.offsets.ensure(n) && b.err.ensure(n)))
    return sfail(h, NZ_ERR_HIP, "device allocation failed (openings)");
  std::vector<int32_t> err(n, 0);
  if (depth > 0) S_HIP(h, hipMemcpyAsync(b.actions.get(), frontier_host, (size_t)n * depth * sizeof(int32_t), hipMemcpyHostToDevice, s));
  const nz::OpeningGames og = opening_games(h);
  S_HIP(h, opening_expand_launch(og, n, b.actions.get(), depth, h->p.max_moves, b.counts.get(), nullptr, 0, nullptr, nullptr, nullptr,
                                 b.err.get(), s));
  S_HIP(h, hipMemcpyAsync(counts_host, b.counts.get(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  S_HIP(h, hipMemcpyAsync(err.data(), b.err.get(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  S_HIP(h, hipStreamSynchronize(s));
  for (int f = 0; f < n; ++f)
    if (err[f]) {
      const int ply = opening_err_ply(err[f]);
      return sfail(h, NZ_ERR_ARG, "prefix %d, ply %d: action %d: %s", f, ply, ply < depth ? frontier_host[(size_t)f * depth + ply] : -1,
                   opening_reason(err[f]));
    }
  if (!children_host) return NZ_OK;
  std::vector<int32_t> offsets(n);
  int64_t total = 0;
  for (int f = 0; f < n; ++f) {                  // the exclusive scan
    offsets[f] = (int32_t)total;
    total += counts_host[f];
    if (total * (depth + 1) > (int64_t)1 << 30) return sfail(h, NZ_ERR_OVERFLOW, "more than 2^30 entries of child prefixes");
  }
  if (total == 0) return NZ_OK;
  if (!(b.children.ensure((size_t)total * (depth + 1)) && b.keys.ensure((size_t)total * 2) &&
        b.planes.ensure((size_t)n * h->host_rules.channels * h->host_rules.tiles)))
    return sfail(h, NZ_ERR_HIP, "device allocation failed (%lld child prefixes)", (long long)total);
  S_HIP(h, hipMemcpyAsync(b.offsets.get(), offsets.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  S_HIP(h, opening_expand_launch(og, n, b.actions.get(), depth, h->p.max_moves, b.counts.get(), b.offsets.get(), (int)total, b.children.get(),
                                 b.keys.get(), b.planes.get(), b.err.get(), s));
  S_HIP(h, hipMemcpyAsync(children_host, b.children.get(), (size_t)total * (depth + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  S_HIP(h, hipMemcpyAsync(keys_host, b.keys.get(), (size_t)total * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  S_HIP(h, hipStreamSynchronize(s));
  return NZ_OK;
}
