// numpy's legacy RandomState (MT19937) stepped by one wavefront: the state's 624 words in LDS, its position in every
// lane's registers, all 64 lanes making the same (wave-uniform) draws.  Shared by the per-game map draw (scs_draw.hip)
// and the random evaluation agent (scs_agents.hip), which keeps each match's state in HBM between its decisions.
//   * init_genrand for an integer seed (rng_host.cpp's seed_state), the twist, tempering;
//   * random_sample = the 53-bit double (a >> 5, b >> 6);
//   * legacy randint(0, n) (choice(range(n)) without p): masked rejection on 32-bit words, n == 1 consumes nothing.
// The kernels that include this run ONE wavefront per workgroup: the twist meets at __syncthreads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nz {

constexpr int MT_N = 624, MT_M = 397;
// Bound of the rejection loop: a masked attempt succeeds with probability > 1/2, so a valid draw never gets there;
// reaching it is reported (mt_randint returns -1) instead of spinning.
constexpr int MT_RANDINT_TRIES = 256;

// The state lives in LDS (key) and in every lane's registers (pos); all lanes step it identically.
struct Mt {
  uint32_t* key;
  int pos;
  int lane;
};

// init_genrand (a serial recurrence: one lane); the callers meet before the first draw
__device__ inline void mt_seed(uint32_t* key, uint32_t seed, int lane) {
  if (lane == 0) {
    uint32_t s = seed;
    for (int i = 0; i < MT_N; ++i) {
      key[i] = s;
      s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)i + 1u;
    }
  }
}

// The MT19937 twist over the wavefront: word i needs the old i + 1 and, for i < 227, the old i + 397, else the NEW
// i - 227 (and word 623 the new word 0).  In 64-word chunks taken in order, every read of a chunk sees the right
// generation when all of the chunk's reads come before its writes: i + 397 is not yet rewritten, i - 227 lies in an
// earlier chunk.
__device__ inline void mt_twist(uint32_t* k, int lane) {
  for (int c = 0; c < MT_N; c += 64) {
    const int i = c + lane;
    uint32_t v = 0;
    if (i < MT_N) {
      const uint32_t y = (k[i] & 0x80000000u) | (k[i + 1 < MT_N ? i + 1 : 0] & 0x7fffffffu);
      v = k[i < MT_N - MT_M ? i + MT_M : i - (MT_N - MT_M)] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    __syncthreads();
    if (i < MT_N) k[i] = v;
    __syncthreads();
  }
}

__device__ inline uint32_t mt_u32(Mt& m) {
  if (m.pos == MT_N) {
    mt_twist(m.key, m.lane);
    m.pos = 0;
  }
  uint32_t y = m.key[m.pos++];
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

__device__ inline double mt_double(Mt& m) {
  const uint32_t a = mt_u32(m) >> 5, b = mt_u32(m) >> 6;
  return (a * 67108864.0 + b) / 9007199254740992.0;
}

// legacy randint(0, n) (choice(range(n))): -1 when the attempts ran out
__device__ inline int mt_randint(Mt& m, int n) {
  if (n <= 1) return 0;
  const uint32_t rng = (uint32_t)(n - 1);
  uint32_t mask = rng;
  mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
  for (int t = 0; t < MT_RANDINT_TRIES; ++t) {
    const uint32_t v = mt_u32(m) & mask;
    if (v <= rng) return (int)v;
  }
  return -1;
}

// ---- streams kept in HBM (mt_keys [n][624], mt_pos [n]) between a wavefront's visits ---------------------------------
// One stream's keys between HBM and the wavefront's LDS copy (key [624], 16-byte aligned as the rows of mt_keys are).
static_assert(MT_N % 4 == 0, "keys are copied in 16-byte words");
__device__ __forceinline__ void mt_copy_keys(uint32_t* dst, const uint32_t* src, int lane) {
  const uint4* s = reinterpret_cast<const uint4*>(src);
  uint4* d = reinterpret_cast<uint4*>(dst);
  for (int i = lane; i < MT_N / 4; i += 64) d[i] = s[i];
}
__device__ __forceinline__ void mt_load_keys(uint32_t* key, const uint32_t* mt_keys, int64_t g, int lane) {
  mt_copy_keys(key, mt_keys + (size_t)g * MT_N, lane);
}
__device__ __forceinline__ void mt_store_keys(uint32_t* mt_keys, int64_t g, const uint32_t* key, int lane) {
  mt_copy_keys(mt_keys + (size_t)g * MT_N, key, lane);
}

// randint(0, n) on stream g, through the LDS copy `key`: the keys go back only if the draw twisted them, the position
// always.  -1 as mt_randint.  The wavefront meets after the load and after the draw.  (Inlined by force: left to the
// compiler it became a real call in agent_act_kernel, with the registers and hidden kernel arguments a call brings.)
__device__ __forceinline__ int mt_stream_randint(uint32_t* key, uint32_t* mt_keys, int32_t* mt_pos, int64_t g, int n, int lane) {
  mt_load_keys(key, mt_keys, g, lane);
  __syncthreads();
  const int pos0 = mt_pos[g];
  Mt m{key, pos0, lane};
  const int k = mt_randint(m, n);
  __syncthreads();
  // at most MT_RANDINT_TRIES < 624 words are drawn: the position went down exactly when the state was twisted
  if (m.pos < pos0) mt_store_keys(mt_keys, g, key, lane);
  if (lane == 0) mt_pos[g] = m.pos;
  return k;
}

// The random agents' streams (scs_agents.hip, ttt_agents.hip): match g = RandomState(seeds[g]) (pos = 624: the first
// draw twists).  Defined in scs_agents.hip.
hipError_t agent_seed_launch(const uint32_t* seeds, uint32_t* mt_keys, int32_t* mt_pos, int n, hipStream_t stream);

}  // namespace nz
