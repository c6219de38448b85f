// Compact SCS replay buffer on the device (C ABI nz_scs_replay_*): a position is stored as the GAME STATE it was, and
// the training batch is rendered inside the gather kernel.
//
// The dense buffer (replay.hip) keeps {state image [C*H*W] f32, policy [A] f32, value, game index} per slot: 10.7 KB on
// a 5x5 board, 42.8 KB on 10x10, times window x the engine's bound on a game's decisions.  Here a slot is one
// self-contained record ("states as compact game state re-rendered"):
//
//   int32 n_children, float value, int32 game_index                       12 bytes
//   float terrain[tiles][3]     the game's own map, as the image's values  12 per tile
//   {int32 action, float policy}[max_children]   the root's child list     8 per child
//   ScsState                    the state before the move                  640 bytes
//   int8 vp[2 * tiles]          victory points as tile indices, player one's first (n_vp of the description in use)
//
// The map is inline on purpose: ReplayIndex.shuffle permutes the buffer and eviction then removes positions of any
// game in any order, so a per-game map table would need reference counts to save about 1 KB per position.
//
// Which slot a position takes and which slots a batch reads is decided on the host (nuzero_amd/replay_device.py
// ReplayIndex, unchanged); the kernels below replay the recorded actions of a finished round through the device rules
// (scs_wave.hpp: scs_admit_wave, scs_dev.hpp: scs_step_wave), one wavefront per game, and render batch rows
// (scs_state_image_wave), one wavefront per row.  Policy targets are formed exactly as replay.hip's append_kernel
// forms them: (float)((double)visit / (double)sum of visits), 0 for a zero visit count.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nuzero_amd.h"
#include "hip_own.hpp"
#include "scs_wave.hpp"

using namespace nz;

namespace {
constexpr int NDESC = 16;                                      // game descriptions per buffer (game_index 0 .. 15)

struct RecLayout {                                             // byte offsets inside a record (all multiples of 4)
  int32_t terrain, children, state, vp, bytes;
};
RecLayout rec_layout(int tiles, int max_children) {
  RecLayout l;
  l.terrain = 12;
  l.children = l.terrain + 12 * tiles;
  l.state = l.children + 8 * max_children;
  l.vp = l.state + (int)sizeof(ScsState);
  l.bytes = (l.vp + 2 * tiles + 3) & ~3;
  return l;
}
// A record is 4-byte aligned and no more (its size is any multiple of 4), so whatever goes into or comes out of one is
// copied in 4-byte words (wave_copy<uint32_t>), and the LDS state at the other end is declared that wide.
}  // namespace

struct nz_scs_replay {
  int device = 0;
  int64_t capacity = 0;
  int32_t max_children = 0, channels = 0, rows = 0, cols = 0, planes = 0;
  RecLayout lay{};
  DevBuf<unsigned char> records;            // [capacity][lay.bytes]
  DevBuf<ScsRules> descs;                   // [NDESC] the registered descriptions
  DevBuf<unsigned long long> first_bad;     // nz_scs_replay_check_games: the smallest (game, move, code) that failed
  DevBuf<int32_t> error_flag;               // the kernels' sticky error word
  std::vector<ScsRules> host_descs = std::vector<ScsRules>(NDESC);
  uint32_t registered = 0;                  // bit i: game_index i has a description
  std::string error;
};

namespace {
thread_local std::string g_err;
nz_status rfail(nz_scs_replay* h, nz_status code, const char* fmt, ...) {
  char buf[384];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) h->error = buf; else g_err = buf;
  return code;
}
#define R_HIP(h, call)                                                                             \
  do {                                                                                             \
    hipError_t e__ = (call);                                                                       \
    if (e__ != hipSuccess) return rfail((h), NZ_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e__)); \
  } while (0)

// what a replay can find wrong with a game's record, in the order a move is checked
enum : int { BAD_LENGTH = 1, BAD_ENDED = 2, BAD_RANGE = 3, BAD_ILLEGAL = 4, BAD_OUTCOME = 5 };
// error word: 1 slot beyond capacity, 2 child count or child action out of range, 4 batch slot out of range,
// 8 nz_scs_replay_save met a record nz_scs_replay_check_games would have refused, 16 a slot's game index has no description,
// 32 a slot's state or map points outside the board (the slot was never saved, or came from a damaged checkpoint)
enum : int { FLAG_SLOT = 1, FLAG_CHILD = 2, FLAG_BATCH = 4, FLAG_RECORD = 8, FLAG_DESC = 16, FLAG_DAMAGED = 32 };

struct ReplayArgs {
  const ScsRules* desc;          // the description registered under game_index
  const int32_t* actions;        // [G][max_moves]
  const int32_t* lengths;        // [G]
  const int32_t* outcomes;       // [G]
  const float* terrain;          // [G][tiles][3] or nullptr: the description's map
  const int32_t* vp;             // [G][n_vp0 + n_vp1][2]
  const int32_t* child_action;   // save: [G][max_moves][round_children]
  const int32_t* child_visit;
  const int32_t* n_children;     // save: [G][max_moves]
  const int64_t* dst_slot;       // save: [G][dst_stride], -1: not stored
  unsigned char* records;
  int64_t capacity;
  int32_t max_moves, round_children, dst_stride, game_index;
  RecLayout lay;
  unsigned long long* first_bad;
  int32_t* error_flag;
};

// One wavefront per game: the rules row is built in LDS (description + the game's own map), then every recorded action
// is checked against the legal mask BEFORE it is stepped -- a damaged record is a reported error, never a step on an
// illegal action.  SAVE: the record of move m goes to dst_slot[g][m].
template <bool SAVE>
__global__ __launch_bounds__(64) void scs_replay_kernel(ReplayArgs a) {
  __shared__ ScsRules R;
  __shared__ __align__(4) ScsState S;
  __shared__ uint32_t mask[SCS_MASK_WORDS];
  const int g = blockIdx.x, lane = threadIdx.x;
  wave_copy<uint32_t>(&R, a.desc, lane);
  __syncthreads();
  if (lane == 0) {
    if (a.terrain != nullptr)
      scs_apply_map(&R, a.terrain + (size_t)g * R.tiles * 3, a.vp + (size_t)g * (R.n_vp[0] + R.n_vp[1]) * 2);
    Scs(R, S).reset();
  }
  __syncthreads();
  const int T = R.tiles, A = R.planes * T, nv0 = R.n_vp[0], nv = nv0 + R.n_vp[1];
  auto bad = [&](int move, int code) {
    if (lane != 0) return;
    if (SAVE) atomicOr(a.error_flag, FLAG_RECORD);
    else atomicMin(a.first_bad, ((unsigned long long)(uint32_t)g << 32) | ((unsigned long long)(uint32_t)move << 8) | (unsigned)code);
  };
  const int len = a.lengths[g];
  if (len < 0 || len > a.max_moves) { bad(0, BAD_LENGTH); return; }
  for (int m = 0; m < len; ++m) {
    const int act = __builtin_amdgcn_readfirstlane(a.actions[(size_t)g * a.max_moves + m]);
    if (const int refused = scs_admit_wave(R, S, mask, act, A, lane)) {   // (wave-uniform: the state is the same LDS for every lane)
      bad(m, refused == SCS_ADMIT_GAME_OVER ? BAD_ENDED : refused == SCS_ADMIT_RANGE ? BAD_RANGE : BAD_ILLEGAL);
      return;
    }
    if constexpr (SAVE) {
      const int64_t slot = m < a.dst_stride ? a.dst_slot[(size_t)g * a.dst_stride + m] : -1;
      if (slot >= a.capacity) {
        if (lane == 0) atomicOr(a.error_flag, FLAG_SLOT);
      } else if (slot >= 0) {
        unsigned char* rec = a.records + (size_t)slot * a.lay.bytes;
        wave_copy<uint32_t>(reinterpret_cast<ScsState*>(rec + a.lay.state), &S, lane);
        float* tr = reinterpret_cast<float*>(rec + a.lay.terrain);
        for (int i = lane; i < 3 * T; i += 64) tr[i] = (&R.terrain_f[0][0])[i];
        int8_t* v = reinterpret_cast<int8_t*>(rec + a.lay.vp);
        for (int i = lane; i < nv; i += 64) v[i] = i < nv0 ? R.vp[0][i] : R.vp[1][i - nv0];
        // the root's children: lanes stride over the list (a node can have more than 64)
        const size_t row = (size_t)g * a.max_moves + m;
        int k = a.n_children[row];
        if (k < 0 || k > a.round_children) {
          if (lane == 0) atomicOr(a.error_flag, FLAG_CHILD);
          k = 0;
        }
        const int32_t* ca = a.child_action + row * a.round_children;
        const int32_t* cv = a.child_visit + row * a.round_children;
        long long part = 0;                                   // an integer sum: exact in any order
        for (int i = lane; i < k; i += 64) part += cv[i];
        for (int o = 32; o; o >>= 1) part += __shfl_xor(part, o, 64);
        const double total = (double)part;
        int32_t* ch = reinterpret_cast<int32_t*>(rec + a.lay.children);
        for (int i = lane; i < k; i += 64) {
          int c = ca[i];
          const int visit = cv[i];
          if (c < 0 || c >= A) {                              // skipped by the gather, as append_kernel skips it
            atomicOr(a.error_flag, FLAG_CHILD);
            c = -1;
          }
          ch[2 * i] = c;
          ch[2 * i + 1] = __builtin_bit_cast(int32_t, visit ? (float)((double)visit / total) : 0.0f);
        }
        if (lane == 0) {
          int32_t* head = reinterpret_cast<int32_t*>(rec);
          head[0] = k;
          head[1] = __builtin_bit_cast(int32_t, (float)a.outcomes[g]);
          head[2] = a.game_index;
        }
      }
    }
    scs_step_wave(R, S, act, lane);
  }
  // a game stopped before its end (a cap on the decisions) is accepted as it is
  if (S.terminal && (int)S.terminal_value != a.outcomes[g]) bad(len, BAD_OUTCOME);
}

struct GatherArgs {
  const unsigned char* records;
  const ScsRules* descs;         // [NDESC]
  const int64_t* slots;          // [B]
  float* out_states; float* out_policies; float* out_values; int32_t* out_game_index;
  int64_t capacity;
  uint32_t registered;
  int32_t max_children;
  RecLayout lay;
  int32_t* error_flag;
};

// One wavefront per batch row: the slot's game index picks the description, the record supplies the map and the state,
// and the image is rendered straight into the batch tensor.
__global__ __launch_bounds__(64) void scs_gather_kernel(GatherArgs a) {
  __shared__ ScsRules R;
  __shared__ __align__(4) ScsState S;
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t slot = a.slots[b];
  if (slot < 0 || slot >= a.capacity) {
    if (lane == 0) atomicOr(a.error_flag, FLAG_BATCH);
    return;
  }
  const unsigned char* rec = a.records + (size_t)slot * a.lay.bytes;
  const int32_t* head = reinterpret_cast<const int32_t*>(rec);
  const int gi = __builtin_amdgcn_readfirstlane(head[2]);
  if (gi < 0 || gi >= NDESC || !((a.registered >> gi) & 1u)) {
    if (lane == 0) atomicOr(a.error_flag, FLAG_DESC);
    return;
  }
  const ScsRules* D = a.descs + gi;
  const int T = D->tiles, A = D->planes * T, nv0 = D->n_vp[0], nv = nv0 + D->n_vp[1];
  if (a.out_states != nullptr) {
    // the rules row of this position: the description, with the record's map over terrain_f and vp (all the image reads
    // of a map; attack_mod / defense_mod / cost are the rules' and stay the description's)
    wave_copy<uint32_t>(&R, D, lane);
    wave_copy<uint32_t>(&S, reinterpret_cast<const ScsState*>(rec + a.lay.state), lane);
    __syncthreads();
    const float* tr = reinterpret_cast<const float*>(rec + a.lay.terrain);
    for (int i = lane; i < 3 * T; i += 64) (&R.terrain_f[0][0])[i] = tr[i];
    const int8_t* v = reinterpret_cast<const int8_t*>(rec + a.lay.vp);
    // Everything the image addresses a tile or a unit with comes out of the record: a record that was never written
    // by the save kernel (a damaged checkpoint) must not turn into a store outside the batch row.
    bool ok = true;
    for (int i = lane; i < nv; i += 64) {
      ok = ok && v[i] >= 0 && v[i] < T;
      if (i < nv0) R.vp[0][i] = v[i]; else R.vp[1][i - nv0] = v[i];
    }
    const int n_att = S.n_attackers;
    if (lane < SCS_MAX_UNITS)
      ok = ok && S.tile[lane] < T && (lane >= n_att || (S.attackers[lane] >= 0 && S.attackers[lane] < SCS_MAX_UNITS));
    ok = ok && S.target < T && n_att >= 0 && n_att <= SCS_MAX_UNITS;
    if (__ballot(!ok) != 0ull) {
      if (lane == 0) atomicOr(a.error_flag, FLAG_DAMAGED);
      return;
    }
    __syncthreads();
    scs_state_image_wave<false>(R, S, a.out_states + (size_t)b * R.channels * T, 0, lane);
  }
  if (a.out_policies != nullptr) {
    float* pol = a.out_policies + (size_t)b * A;
    for (int i = lane; i < A; i += 64) pol[i] = 0.0f;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");    // the scattered entries land after the fill
    __syncthreads();
    int k = head[0];
    if (k < 0 || k > a.max_children) {
      if (lane == 0) atomicOr(a.error_flag, FLAG_CHILD);
      k = 0;
    }
    const int32_t* ch = reinterpret_cast<const int32_t*>(rec + a.lay.children);
    for (int i = lane; i < k; i += 64) {
      const int c = ch[2 * i];
      if (c >= 0 && c < A) pol[c] = __builtin_bit_cast(float, ch[2 * i + 1]);
    }
  }
  if (lane == 0) {
    if (a.out_values) a.out_values[b] = __builtin_bit_cast(float, head[1]);
    if (a.out_game_index) a.out_game_index[b] = gi;
  }
}

// the shape of a description as a buffer sees it; false (and a message) where the library cannot hold it
bool desc_rules(const nz_scs_desc* d, ScsRules* out, std::string* err) {
  if (!scs_fill_rules(d, out, err)) return false;
  if (out->n_vp[0] > out->tiles || out->n_vp[1] > out->tiles) {
    *err = "more victory points than tiles";
    return false;
  }
  return true;
}
}  // namespace

extern "C" {

const char* nz_scs_replay_last_error(const nz_scs_replay* h) { return h ? h->error.c_str() : g_err.c_str(); }

int64_t nz_scs_replay_record_bytes(const nz_scs_desc* desc, int32_t max_children) {
  if (!desc) { rfail(nullptr, NZ_ERR_ARG, "null argument"); return -1; }
  ScsRules r;
  std::string err;
  if (!desc_rules(desc, &r, &err)) { rfail(nullptr, NZ_ERR_ARG, "%s", err.c_str()); return -1; }
  const int bound = scs_children_bound(r);
  if (max_children <= 0) max_children = (bound + 63) / 64 * 64;        // as the search engine rounds it
  if (max_children < bound) {
    rfail(nullptr, NZ_ERR_ARG, "a position of this game can have %d children, the records would hold %d", bound, max_children);
    return -1;
  }
  return rec_layout(r.tiles, max_children).bytes;
}

nz_status nz_scs_replay_create(nz_scs_replay** out, int64_t capacity, int32_t max_children, int32_t channels, int32_t rows,
                               int32_t cols, int32_t num_actions, int32_t device) {
  if (!out) return rfail(nullptr, NZ_ERR_ARG, "null argument");
  *out = nullptr;
  const int stacking = (channels - 48) / 19, planes = 3 + 9 * stacking;
  if (capacity <= 0 || max_children <= 0 || max_children > (1 << 16) || rows <= 0 || cols <= 0 || rows * cols > SCS_MAX_TILES)
    return rfail(nullptr, NZ_ERR_ARG, "bad sizes");
  if (stacking < 1 || stacking > SCS_MAX_STACK || channels != 48 + 19 * stacking || num_actions != planes * rows * cols)
    return rfail(nullptr, NZ_ERR_ARG, "%d channels and %d actions on %d x %d tiles are not an SCS image shape", channels,
                 num_actions, rows, cols);
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
    return rfail(nullptr, NZ_ERR_HIP, "no HIP device %d (no CPU fallback)", device);
  (void)hipSetDevice(device);
  nz_scs_replay* h = new nz_scs_replay;
  h->device = device; h->capacity = capacity; h->max_children = max_children;
  h->channels = channels; h->rows = rows; h->cols = cols; h->planes = planes;
  h->lay = rec_layout(rows * cols, max_children);
  if (!h->records.ensure((size_t)capacity * h->lay.bytes) || !h->descs.ensure(NDESC) || !h->first_bad.ensure(1) ||
      !h->error_flag.ensure(1)) {
    nz_scs_replay_destroy(h);
    return rfail(nullptr, NZ_ERR_HIP, "device allocation failed (%lld positions of %d bytes)", (long long)capacity, h->lay.bytes);
  }
  // (slots read as an empty board until they are saved)
  if (hipMemset(h->records.get(), 0, (size_t)capacity * h->lay.bytes) != hipSuccess ||
      hipMemset(h->error_flag.get(), 0, sizeof(int32_t)) != hipSuccess) {
    nz_scs_replay_destroy(h);
    return rfail(nullptr, NZ_ERR_HIP, "memset failed");
  }
  *out = h;
  return NZ_OK;
}

void nz_scs_replay_destroy(nz_scs_replay* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  delete h;
}

nz_status nz_scs_replay_dims(const nz_scs_replay* h, int64_t* capacity, int32_t* record_bytes, int32_t* max_children,
                             int32_t* num_actions) {
  if (!h) return NZ_ERR_ARG;
  if (capacity) *capacity = h->capacity;
  if (record_bytes) *record_bytes = h->lay.bytes;
  if (max_children) *max_children = h->max_children;
  if (num_actions) *num_actions = h->planes * h->rows * h->cols;
  return NZ_OK;
}

nz_status nz_scs_replay_register(nz_scs_replay* h, int32_t game_index, const nz_scs_desc* desc) {
  if (!h || !desc) return rfail(h, NZ_ERR_ARG, "null argument");
  if (game_index < 0 || game_index >= NDESC) return rfail(h, NZ_ERR_ARG, "game index %d: 0 .. %d", game_index, NDESC - 1);
  ScsRules r;
  std::string err;
  if (!desc_rules(desc, &r, &err)) return rfail(h, NZ_ERR_ARG, "%s", err.c_str());
  if (r.rows != h->rows || r.cols != h->cols || r.planes != h->planes || r.channels != h->channels)
    return rfail(h, NZ_ERR_ARG, "a description of %d x %d tiles, %d planes and %d channels in a buffer of %d x %d, %d and %d",
                 r.rows, r.cols, r.planes, r.channels, h->rows, h->cols, h->planes, h->channels);
  const int bound = scs_children_bound(r);
  if (bound > h->max_children)
    return rfail(h, NZ_ERR_ARG, "a position of this game can have %d children, the buffer's records hold %d", bound, h->max_children);
  if ((h->registered >> game_index) & 1u) {
    if (memcmp(&h->host_descs[game_index], &r, sizeof(r)) != 0)
      return rfail(h, NZ_ERR_ARG, "game index %d already has a different description", game_index);
    return NZ_OK;
  }
  R_HIP(h, hipSetDevice(h->device));
  R_HIP(h, hipMemcpy(h->descs.get() + game_index, &r, sizeof(r), hipMemcpyHostToDevice));
  h->host_descs[game_index] = r;
  h->registered |= 1u << game_index;
  return NZ_OK;
}

static nz_status replay_args(nz_scs_replay* h, int32_t game_index, int64_t n_games, const int32_t* actions, int32_t max_moves,
                             const int32_t* lengths, const int32_t* outcomes, const float* terrain, const int32_t* vp,
                             ReplayArgs* a) {
  if (!h || !actions || !lengths || !outcomes) return rfail(h, NZ_ERR_ARG, "null argument");
  if (game_index < 0 || game_index >= NDESC || !((h->registered >> game_index) & 1u))
    return rfail(h, NZ_ERR_ARG, "game index %d has no description (nz_scs_replay_register)", game_index);
  if ((terrain != nullptr) != (vp != nullptr)) return rfail(h, NZ_ERR_ARG, "a game's map is terrain and victory points");
  if (max_moves <= 0 || n_games < 0 || n_games > 0x7fffffff) return rfail(h, NZ_ERR_ARG, "bad sizes");
  *a = ReplayArgs{};
  a->desc = h->descs.get() + game_index;
  a->actions = actions; a->lengths = lengths; a->outcomes = outcomes; a->terrain = terrain; a->vp = vp;
  a->records = h->records.get(); a->capacity = h->capacity;
  a->max_moves = max_moves; a->game_index = game_index; a->lay = h->lay;
  a->first_bad = h->first_bad.get(); a->error_flag = h->error_flag.get();
  return NZ_OK;
}

nz_status nz_scs_replay_check_games(nz_scs_replay* h, int32_t game_index, int64_t n_games, const int32_t* actions_dev,
                                    int32_t max_moves, const int32_t* lengths_dev, const int32_t* outcomes_dev,
                                    const float* terrain_dev, const int32_t* vp_dev, void* stream) {
  ReplayArgs a;
  const nz_status st = replay_args(h, game_index, n_games, actions_dev, max_moves, lengths_dev, outcomes_dev, terrain_dev, vp_dev, &a);
  if (st != NZ_OK || n_games == 0) return st;
  const hipStream_t s = (hipStream_t)stream;
  R_HIP(h, hipSetDevice(h->device));
  R_HIP(h, hipMemsetAsync(a.first_bad, 0xff, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(scs_replay_kernel<false>, dim3((unsigned)n_games), dim3(64), 0, s, a);
  R_HIP(h, hipGetLastError());
  unsigned long long bad = 0;
  R_HIP(h, hipMemcpyAsync(&bad, a.first_bad, sizeof(bad), hipMemcpyDeviceToHost, s));
  R_HIP(h, hipStreamSynchronize(s));
  if (bad == ~0ull) return NZ_OK;
  const int g = (int)(bad >> 32), m = (int)((bad >> 8) & 0xffffff), code = (int)(bad & 0xff);
  const char* what = code == BAD_LENGTH    ? "the recorded length is outside 0 .. max_moves"
                     : code == BAD_ENDED   ? "the game had ended before this recorded move"
                     : code == BAD_RANGE   ? "the recorded action is outside 0 .. A-1"
                     : code == BAD_ILLEGAL ? "the recorded action is not legal in this position"
                                           : "the game ended with another outcome than the recorded one";
  return rfail(h, NZ_ERR_ARG, "game %d, move %d: %s (nothing was stored)", g, m, what);
}

nz_status nz_scs_replay_save(nz_scs_replay* h, int32_t game_index, int64_t n_games, const int32_t* actions_dev,
                             int32_t max_moves, const int32_t* lengths_dev, const int32_t* outcomes_dev,
                             const float* terrain_dev, const int32_t* vp_dev, const int32_t* child_action_dev,
                             const int32_t* child_visit_dev, const int32_t* n_children_dev, int32_t round_children,
                             const int64_t* dst_slot_dev, int32_t dst_stride, void* stream) {
  ReplayArgs a;
  const nz_status st = replay_args(h, game_index, n_games, actions_dev, max_moves, lengths_dev, outcomes_dev, terrain_dev, vp_dev, &a);
  if (st != NZ_OK) return st;
  if (!child_action_dev || !child_visit_dev || !n_children_dev || !dst_slot_dev) return rfail(h, NZ_ERR_ARG, "null argument");
  if (round_children <= 0 || round_children > h->max_children)
    return rfail(h, NZ_ERR_ARG, "child lists of %d entries, the buffer's records hold %d", round_children, h->max_children);
  if (dst_stride < 0) return rfail(h, NZ_ERR_ARG, "bad sizes");
  if (n_games == 0 || dst_stride == 0) return NZ_OK;
  a.child_action = child_action_dev; a.child_visit = child_visit_dev; a.n_children = n_children_dev;
  a.round_children = round_children; a.dst_slot = dst_slot_dev; a.dst_stride = dst_stride;
  R_HIP(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(scs_replay_kernel<true>, dim3((unsigned)n_games), dim3(64), 0, (hipStream_t)stream, a);
  R_HIP(h, hipGetLastError());
  return NZ_OK;
}

nz_status nz_scs_replay_gather(nz_scs_replay* h, const int64_t* slots_dev, int64_t batch, float* states_out,
                               float* policies_out, float* values_out, int32_t* game_index_out, void* stream) {
  if (!h || !slots_dev) return rfail(h, NZ_ERR_ARG, "null argument");
  if (batch <= 0) return NZ_OK;
  R_HIP(h, hipSetDevice(h->device));
  GatherArgs a{h->records.get(), h->descs.get(), slots_dev, states_out, policies_out, values_out, game_index_out,
               h->capacity, h->registered, h->max_children, h->lay, h->error_flag.get()};
  hipLaunchKernelGGL(scs_gather_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, a);
  R_HIP(h, hipGetLastError());
  return NZ_OK;
}

nz_status nz_scs_replay_check(nz_scs_replay* h, void* stream) {
  if (!h) return rfail(nullptr, NZ_ERR_ARG, "null argument");
  R_HIP(h, hipSetDevice(h->device));
  int32_t f = 0;
  R_HIP(h, hipMemcpyAsync(&f, h->error_flag.get(), sizeof(f), hipMemcpyDeviceToHost, (hipStream_t)stream));
  R_HIP(h, hipStreamSynchronize((hipStream_t)stream));
  if (f) return rfail(h, NZ_ERR_OVERFLOW, "device check failed (flag %d: 1 slot beyond capacity, 2 child count or action out "
                                          "of range, 4 batch slot out of range, 8 unchecked record, 16 game index without "
                                          "a description, 32 damaged record)", f);
  return NZ_OK;
}

nz_status nz_scs_replay_export_slots(nz_scs_replay* h, int64_t n, void* bytes_dev, void* stream) {
  if (!h || (!bytes_dev && n > 0)) return rfail(h, NZ_ERR_ARG, "null argument");
  if (n < 0 || n > h->capacity) return rfail(h, NZ_ERR_ARG, "%lld slots of a buffer of %lld", (long long)n, (long long)h->capacity);
  if (n == 0) return NZ_OK;
  R_HIP(h, hipSetDevice(h->device));
  R_HIP(h, hipMemcpyAsync(bytes_dev, h->records.get(), (size_t)n * h->lay.bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return NZ_OK;
}

nz_status nz_scs_replay_import_slots(nz_scs_replay* h, int64_t n, const void* bytes_dev, void* stream) {
  if (!h || (!bytes_dev && n > 0)) return rfail(h, NZ_ERR_ARG, "null argument");
  if (n < 0 || n > h->capacity) return rfail(h, NZ_ERR_ARG, "%lld slots of a buffer of %lld", (long long)n, (long long)h->capacity);
  if (n == 0) return NZ_OK;
  R_HIP(h, hipSetDevice(h->device));
  R_HIP(h, hipMemcpyAsync(h->records.get(), bytes_dev, (size_t)n * h->lay.bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return NZ_OK;
}

}  // extern "C"
