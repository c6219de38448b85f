// Internal declarations shared by the engine's translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nuzero_amd.h"

namespace nz {

constexpr int TTT_ACTIONS = 9;
constexpr int TTT_MAX_MOVES = 9;
constexpr int TTT_TABLE_ROWS = 19683;   // 3^9
constexpr int MAX_PATH = 16;            // TTT depth <= 9 plus the root
constexpr int LANES_PER_GAME = 16;      // one 16-lane DPP row per game tree

// node link word y: n_children[0:12) | action[12:24) | to_play[24:28) | term[28:32)
constexpr uint32_t TO_PLAY_UNSET = 15u;
__host__ __device__ inline uint32_t pack_meta(uint32_t n_children, uint32_t action, uint32_t to_play,
                                              uint32_t term) {
  return n_children | (action << 12) | (to_play << 24) | (term << 28);
}
__host__ __device__ inline uint32_t meta_children(uint32_t m) { return m & 0xfffu; }
__host__ __device__ inline uint32_t meta_action(uint32_t m) { return (m >> 12) & 0xfffu; }
__host__ __device__ inline uint32_t meta_to_play(uint32_t m) { return (m >> 24) & 0xfu; }

// One tree node (Search/Node.py:3-32), 48 bytes = three 16-byte loads; a node's children are
// contiguous and in ascending action order.
struct __attribute__((aligned(16))) TNode {
  double value_sum;
  double q;               // value_sum / visit, 0.0 while unvisited (Node.value()); rewritten by every backup
  double prior;
  int32_t visit;
  uint32_t first;         // index of the first child
  uint32_t meta;          // packed: see pack_meta
  uint32_t pad[3];
};
static_assert(sizeof(TNode) == 48, "three 16-byte loads per node");

// Everything the tree kernels need, passed by value.
struct TreeParams {
  TNode* nodes;           // [n_slots][cap]
  int32_t cap;
  int32_t n_games;        // games per self-play round (records, random tables)
  int32_t n_slots;        // games in flight at once (tree arenas); lock-step needs n_slots == n_games
  int32_t* next_game;     // work queue head of the persistent kernel
  // per-game state
  uint32_t* board;        // live game: player-one stones | player-two stones << 16
  int32_t* length;
  int32_t* alive;
  int32_t* outcome;
  int32_t* root;
  int32_t* node_count;
  int32_t* sims_left;
  int32_t* pending;       // leaf slot awaiting a network result, or -1
  uint32_t* leaf_board;   // scratch position at the pending leaf
  int32_t* path;          // [G][MAX_PATH]
  int32_t* path_len;
  int32_t* sim_count;
  int32_t* exp_count;
  int32_t* sel_nodes;     // descent levels (internal nodes scored)
  int32_t* sel_children;  // children scored
  int32_t* new_nodes;     // nodes created by the game's expansions (sum of the children counts)
  int32_t* n_root_children;
  int32_t* desync;        // 1: the host's pre-drawn randomness did not fit this game (selfplay.hip)
  // leaf queue feeding the network kernel
  int32_t* leaf_count;    // [2], ping-pong by iteration parity
  uint32_t* leaf_boards;  // [G]
  const float* leaf_logits;  // [G][A]
  const float* leaf_value;   // [G]
  // table evaluator (test hook) or nullptr
  const float* table;
  // search constants
  const double* bias_tab;  // log((N + base + 1) / base) + init, N = 0..tab_len-1
  const double* sqrt_tab;  // sqrt(N)
  int32_t tab_len;
  int32_t sims;
  int32_t negate_player;
  double value_factor;
  double frac, one_minus_frac;
  int32_t training;
  int32_t softmax_moves;
  double eps_softmax, eps_random;
  int32_t sims_per_cycle;  // persistent kernel: simulations a game may run between two network passes
  int32_t slots_per_wg;    // persistent kernel: game slots a workgroup plays (1..16 of its 16 network rows): fewer slots
                           // than 16 x CUs are spread over all CUs rather than packed into a quarter of them
  int32_t burst_under_net; // persistent kernel: 1 = a wavefront whose row hit the per-cycle cap sits out the network pass and
                           // keeps simulating under it while its SIMD partner runs both halves of the tile (selfplay.hip);
                           // 2 = waves 0-3 sit out every pass (test hook for the partner's solo list); 0 = off
  int32_t max_cycles;      // persistent kernel: tree/network cycles a workgroup may run before it gives up
                           // (error flag 64) -- a bound every wave reaches, whatever goes wrong
  int32_t* error_flag;
  // per-move records, [G][T]...
  uint32_t* hist_board;
  int32_t* hist_action;
  int32_t* hist_visits;    // [G][T][A]
  int32_t* hist_tree_size;
  int32_t* hist_children;
  double* hist_bias;
  double* hist_prior;      // [G][T][A]
  double* hist_value_sum;  // [G][T][A]
  double* hist_root_value_sum;
};

// boards: [n_games] start positions (needs n_slots == n_games), or nullptr for the empty board
void launch_reset(const TreeParams& p, const uint32_t* boards, hipStream_t s);
void launch_noise(const TreeParams& p, const double* noise, hipStream_t s);
void launch_advance(const TreeParams& p, int iteration, hipStream_t s);
void launch_finish_move(const TreeParams& p, const double* uniforms, const int32_t* forced, hipStream_t s);
void launch_last_actions(const TreeParams& p, int32_t* actions, hipStream_t s);
void launch_export_states(const TreeParams& p, float* states, hipStream_t s);
void launch_export_visits(const TreeParams& p, int32_t* visits, int32_t* actions, int32_t* tree_size,
                          int32_t* n_children, double* bias, hipStream_t s);

int selfplay_blocks(int n_slots, int slots_per_wg);
// stamps != nullptr selects the diagnostic build ([blocks][4] phase ticks, see selfplay.hip); `packed`: prog_dev is a
// packed program for p.slots_per_wg positions (net_packed_dev.hpp) and the kernel's packed instantiation runs it
void launch_selfplay(const TreeParams& p, const struct NetProgram* prog_dev, int n_layers, const float* weights,
                     const double* noise, const double* uniforms, unsigned long long* stamps, bool packed, hipStream_t s,
                     int prec = NZ_PREC_FLOAT32);   // NZ_PREC_BF16: the plain-bf16 program and stream; never packed, no burst

// ---- network ----------------------------------------------------------------
// Arithmetic of the fused network: net_dev.hpp.  K groups are 32 channels; the packed weights of
// one K group of one 16-channel output tile are [tap][piece][lane][8 bf16].
constexpr int NET_KG_CHANNELS = 32;
constexpr int NET_KG_DWORDS = 9 * 3 * 64 * 4;
// plain-bf16 mode (nz_engine_precision): one rounded bf16 per weight, [tap][lane][8 bf16], a third of the dwords
constexpr int NET_KG_DWORDS_BF16 = 9 * 64 * 4;
constexpr int NET_ACT_BUFFERS = 2;                 // activation buffers in LDS (ping-pong)
constexpr int NET_DST_POLICY = NET_ACT_BUFFERS;    // NetJob::dst: policy logits out
constexpr int NET_DST_VALUE = NET_ACT_BUFFERS + 1; // NetJob::dst: value out
constexpr int NET_DST_STRIP = NET_ACT_BUFFERS + 2; // NetJob::dst: the 16-channel strip (policy head's second tile, net_dev.hpp)
constexpr int NET_SSLOT_SPLIT = -1;                // NetJob::sslot: K group read from src slots 6-7 (quads 0-1) + the strip (2-3)

// The network is compiled on the host into one job list per wave (net_dev.hpp).
// A job is one (conv layer, 16-channel output tile, output-cell group) unit; the
// jobs of a stage are independent, a workgroup barrier separates stages.
struct NetJob {
  int32_t w_off;       // dword offset of this (layer, n-tile)'s packed main weights [kgroup][tap][piece][lane][8 bf16]
                       // (plain-bf16 mode: of that mode's stream, [kgroup][tap][lane][8 bf16]; so next_w_off, first_w_off, wx_off)
  int32_t wx_off;      // float offset of its packed input-plane weights [tap][lane]
  int32_t next_w_off;  // w_off of the next job of this wave that reads weights, or -1 (prefetch target)
  int8_t kgroups;      // 32-channel K groups read from the source activation buffer
  int8_t sslot;        // first 16-byte slot of the K groups in the source rows (0 or 2, 4, 6), or NET_SSLOT_SPLIT
  int16_t nt;          // output tile: channels 16 nt .. 16 nt + 15 (weights, network outputs)
  int8_t extra;        // 1: also read the (<= 4) input planes as one extra K step
  int8_t og;           // output-cell group (net_dev.hpp OG_MASK); OG_NONE = no work, barrier only
  int8_t src, dst;     // activation buffers 0..1; dst NET_DST_POLICY / NET_DST_VALUE = network outputs
  int8_t res;          // residual buffer or -1
  int8_t act;          // 0 none, 1 relu, 2 tanh, 3 elu
  int8_t flags;        // NET_JOB_STAGE_END | NET_JOB_PROGRESSIVE
  int8_t dtile;        // 16-channel tile of the destination rows the epilogue writes (dst a buffer or the strip)
};
constexpr int NET_JOB_STAGE_END = 1;     // NetJob::flags: workgroup barrier after this job
// NetJob::flags: the epilogue of each output cell that is final before the K loop's last tap is issued between the
// MFMAs of the remaining taps (net_dev.hpp ProgEpi).  The cell's LDS rows are then written while the job still reads
// operands, so the host sets it only where no job of the stage reads, as an MFMA operand, an area the job writes.
constexpr int NET_JOB_PROGRESSIVE = 2;
// cells (bit o) of output-cell group og (net_dev.hpp)
__host__ __device__ constexpr int og_mask(int og) {
  return og == 0 ? 0x1FF : og == 1 ? 0x011 : og == 2 ? 0x00A : og == 3 ? 0x0A0 : og == 4 ? 0x144 :
         og == 5 ? 0x02F : og == 6 ? 0x1D0 : 0;
}
// last tap (0..8, tap = 3 (dy + 1) + (dx + 1), input cell = output cell + (dy, dx)) that reaches output cell o of the 3x3 board
__host__ __device__ constexpr int net_final_tap(int o) {
  return 3 * ((o / 3 < 2 ? 1 : 0) + 1) + ((o % 3 < 2 ? 1 : 0) + 1);
}
// The groups the kernel has the progressive form for: the late half {4,6,7,8} and the quarters {5,7} {2,6,8}, whose
// epilogues nothing else on their SIMD covers, and the whole tile of a solo list, which runs alone on its SIMD.  (The
// early half {0,1,2,3,5} has two early cells and three pairs after them, and its epilogue already runs under the late
// half's MFMAs; the other quarters have no early cell.)
__host__ __device__ constexpr bool net_og_progressive(int cells) {
  return cells == 0x1D0 || cells == 0x0A0 || cells == 0x144 || cells == 0x1FF;
}
constexpr int NET_WAVES_HOST = 8;
constexpr int NET_MAX_JOBS = 192;
constexpr int OG_NONE = 7;
constexpr int NET_MAX_SOLO_JOBS = 2 * NET_MAX_JOBS;   // a solo list: two waves' jobs
struct NetProgram {
  int32_t n_jobs[NET_WAVES_HOST];
  int32_t first_w_off[NET_WAVES_HOST];   // w_off of each wave's first weight-reading job, or -1
  NetJob jobs[NET_WAVES_HOST][NET_MAX_JOBS];
  // A stealing pass (net_dev.hpp net_tile, `steal`): wave w ^ 4 sits the pass out and wave w walks solo_jobs[w] instead of
  // its own list -- a plain job list in the same format, with its own next_w_off chain and one stage-end flag per stage.
  // Stage by stage it holds w's jobs and then w ^ 4's; where those are the two cell halves of one tile of one conv into
  // a buffer, one job of group 0 (all nine cells) replaces them (engine.hip compile_net; NZ_BURST_WHOLE_TILE=0: never).
  int32_t solo_n_jobs[NET_WAVES_HOST];
  int32_t solo_first_w[NET_WAVES_HOST];
  NetJob solo_jobs[NET_WAVES_HOST][NET_MAX_SOLO_JOBS];
  int32_t n_stages;
  int32_t stage_budget[NET_MAX_JOBS];    // simulations a sitting-out wave's row may run before the stage's barrier
};

// ---- the packed pass (net_packed_dev.hpp): a network pass for P <= NET_PACKED_MAX positions -------------------------
// The MFMA's 16 columns are (position, cell) pairs instead of positions: pair c = 9 pos + cell sits in column c % 16 of
// column tile c / 16, and for one tap a column's activation fragment is that of input cell cell + (dy, dx) of its
// position (zero where that is off the board), so a conv costs 9 ceil(9 P / 16) six-MFMA chains per K group and output
// tile where the 16-position tile costs 49.  Its program is a NetProgram whose jobs are (conv, output tile, run of
// column tiles): NetJob::og = first column tile + 8 * tiles (OG_NONE: barrier only), src / dst / res are AREAS, and the
// solo lists and stage budgets stay empty (no wave sits a packed pass out).
constexpr int NET_PACKED_MAX = NZ_NET_PACKED_MAX;
constexpr int NET_PACKED_DEFAULT = 4;        // engines of at most this many games per workgroup take it: the measured rule
                                             // (engine.hip nz_engine_create_ex, profiles/r10_packed_pass.txt)
constexpr int NET_PACKED_AREAS = 4;         // areas of 9 P activation rows inside the two activation buffers
constexpr int NET_PACKED_RUN = 2;            // column tiles one job may hold (accumulators, operand fragments)
constexpr int NET_PACKED_DST_POLICY = 8;     // NetJob::dst of a packed job: policy logits out
constexpr int NET_PACKED_DST_VALUE = 9;      // NetJob::dst of a packed job: value out
__host__ __device__ constexpr int net_packed_tiles(int P) { return (9 * P + 15) / 16; }
__host__ __device__ constexpr int net_packed_og(int first_tile, int tiles) { return first_tile + 8 * tiles; }
// source cell of (cell, tap), tap = 3 (dy + 1) + (dx + 1) as for net_final_tap; -1: off the board
__host__ __device__ constexpr int net_packed_tap_source(int cell, int tap) {
  const int y = cell / 3 + tap / 3 - 1, x = cell % 3 + tap % 3 - 1;
  return y >= 0 && y < 3 && x >= 0 && x < 3 ? 3 * y + x : -1;
}

void launch_net(const NetProgram* prog_dev, int n_layers, const float* packed_weights,
                const uint32_t* boards, const float* states, const int32_t* count_dev, int max_positions,
                float* logits, float* value, float* probs, unsigned long long* stamps, hipStream_t s,
                int prec = NZ_PREC_FLOAT32);     // NZ_PREC_BF16: prog_dev and packed_weights are the plain-bf16 mode's
// (net.hip <-> net_bf16.hip) the softmax of launch_net for 9 logits a position; the network kernel of NZ_PREC_BF16
void launch_softmax9(const float* logits, float* probs, int batch, hipStream_t s);
void launch_net_bf16(const NetProgram* prog_dev, const float* bf16_weights, const uint32_t* boards, const float* states,
                     const int32_t* count_dev, int max_positions, float* logits, float* value, unsigned long long* stamps,
                     hipStream_t s);
// plain-bf16 only, the test hook (net_bf16.hip net_dump_kernel): launch_net's outputs and what the device held; the arrays
// hold 16 * ceil(batch / 16) rows
void launch_net_dump(const NetProgram* prog_dev, const float* bf16_weights, const float* states, int batch, float* logits,
                     float* value, float* probs, float* planes, float* acts, int max_stages, float* vcells, hipStream_t s);
// the same outputs from the packed pass: one workgroup per P positions, `prog_dev` a packed program for P
void launch_net_packed(const NetProgram* prog_dev, int P, const float* packed_weights, const float* states, int batch,
                       float* logits, float* value, float* probs, hipStream_t s);

}  // namespace nz
