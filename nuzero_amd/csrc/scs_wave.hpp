// What the one-wavefront-per-game side kernels share (scs_agents.hip, scs_openings.hip, scs_draw.hip, scs_replay.hip):
// the rules row and the game in LDS, scs_dev.hpp's legal mask, step and image on them.  Here:
//   * the copy of a rules row or a state by the wavefront, and the rules row of game g;
//   * the legal set of a position: the mask in LDS, its count, its k-th action in ascending flat index;
//   * the admission of an action from outside: not terminal, in range, bit set in the legal mask -- before any step.
// All 64 lanes call these together; what they return is wave-uniform.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scs_dev.hpp"

namespace nz {

// words of a position's legal mask: one bit per action of the largest game (SCS_MAX_PLANES, scs_dev.hpp)
constexpr int SCS_MASK_WORDS = (SCS_MAX_PLANES * SCS_MAX_TILES + 31) / 32;
static_assert(SCS_MASK_WORDS <= 128, "a lane holds two words of the legal mask");

// *dst = *src in words of type W, the lanes striding over them.  W is the caller's statement about BOTH ends: each is
// aligned to sizeof(W) by its declaration (ScsRules: 8, rules rows in HBM are arrays of it; ScsState: 2 unless the
// __shared__ object is declared wider; the compact replay records: 4 and no more).
template <typename W, typename T>
__device__ __forceinline__ void wave_copy(T* dst, const T* src, int lane) {
  static_assert(sizeof(T) % sizeof(W) == 0, "the object is copied in whole words");
  const W* s = reinterpret_cast<const W*>(src);
  W* d = reinterpret_cast<W*>(dst);
  for (int i = lane; i < (int)(sizeof(T) / sizeof(W)); i += 64) d[i] = s[i];
}

// the rules row game g plays under: one row, or one per game (rules_row, as SearchParams)
__device__ __forceinline__ const ScsRules* rules_of(const ScsRules* rules, const int32_t* rules_row, int g) {
  return rules + (rules_row ? rules_row[g] : 0);
}

// inclusive prefix sum over the wavefront
__device__ __forceinline__ int wave_scan(int v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// The index of the k-th set bit (k < the number of set bits) of the mask whose words `base + lane` the lanes hold in w,
// or -1 when it lies past these 64 words (k is then reduced by their count): ballot and popcount prefix.
__device__ __forceinline__ int kth_set_bit(uint32_t w, int base, int& k, int lane) {
  const int c = __popc(w), inc = wave_scan(c, lane);
  const int total = __shfl(inc, 63, 64);
  if (k >= total) { k -= total; return -1; }
  const int owner = __ffsll((long long)__ballot(inc > k)) - 1;       // the first lane whose words reach past k
  int bit = -1;
  if (lane == owner) {
    uint32_t x = w;
    for (int i = k - (inc - c); i > 0; --i) x &= x - 1;               // (at most 31 rounds)
    bit = (base + lane) * 32 + __ffs((int)x) - 1;
  }
  return __shfl(bit, owner, 64);
}

// The legal actions of a position: the mask in LDS (smask [SCS_MASK_WORDS]), words lane and lane + 64 of it in each
// lane's registers, their count.
struct WaveLegal {
  uint32_t w0, w1;
  int count;
  // the k-th legal action (k < count) in ascending flat index; -1 cannot happen for such a k
  __device__ __forceinline__ int kth(int k, int lane) const {
    const int action = kth_set_bit(w0, 0, k, lane);
    return action >= 0 ? action : kth_set_bit(w1, 64, k, lane);
  }
};
__device__ __forceinline__ WaveLegal wave_legal(const ScsRules& R, const ScsState& sc, uint32_t* smask, int lane) {
  scs_legal_mask_wave<SCS_MASK_WORDS>(R, sc, smask, lane);
  WaveLegal l;
  l.w0 = lane < SCS_MASK_WORDS ? smask[lane] : 0u;
  l.w1 = lane + 64 < SCS_MASK_WORDS ? smask[lane + 64] : 0u;
  l.count = __shfl(wave_scan(__popc(l.w0) + __popc(l.w1), lane), 63, 64);
  return l;
}

// The admission of an action that came from outside (a recorded game, an opening prefix): 0, or what failed first, in
// this order.  The position's legal mask is left in smask [SCS_MASK_WORDS]; nothing is stepped -- the caller steps an
// admitted action and maps a refusal onto the code it reports.  `action` is wave-uniform, as the state in LDS is.
enum : int { SCS_ADMIT_GAME_OVER = 1, SCS_ADMIT_RANGE = 2, SCS_ADMIT_ILLEGAL = 3 };
__device__ __forceinline__ int scs_admit_wave(const ScsRules& R, const ScsState& sc, uint32_t* smask, int action,
                                              int num_actions, int lane) {
  if (sc.terminal) return SCS_ADMIT_GAME_OVER;
  if (action < 0 || action >= num_actions) return SCS_ADMIT_RANGE;   // an action indexes the mask only after this
  scs_legal_mask_wave<SCS_MASK_WORDS>(R, sc, smask, lane);
  if (!((smask[action >> 5] >> (action & 31)) & 1u)) return SCS_ADMIT_ILLEGAL;
  return 0;
}

}  // namespace nz
