/*
 * nuzero_amd.h -- C ABI of the MI355X self-play engine.
 *
 * The reference (guilherme439/NuZero) is pure Python and has no FFI; the
 * boundary this library replaces is the Python contract between the trainer and
 * the self-play worker.  Each entry point names the
 * reference code whose work it takes over.  All paths are relative to the
 * reference repository root.
 *
 * Conventions
 *   - plain C symbols, opaque handle, int status (0 = NZ_OK), no exceptions;
 *   - one engine per GPU, not thread-safe (one Gamer = one single-threaded
 *     actor in the reference, Training/Gamer.py:17-37);
 *   - "dev" pointers are device pointers owned by the caller (PyTorch-ROCm
 *     tensors); "host" pointers are ordinary host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *     work is enqueued on it and is NOT synchronised unless stated.
 */
#ifndef NUZERO_AMD_H
#define NUZERO_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nz_engine nz_engine;
typedef struct nz_rng nz_rng;
typedef int nz_status;

enum {
  NZ_OK = 0,
  NZ_ERR_ARG = 1,        /* bad argument / unsupported configuration */
  NZ_ERR_HIP = 2,        /* a HIP call failed; see nz_last_error */
  NZ_ERR_STATE = 3,      /* call out of order (e.g. search before weights) */
  NZ_ERR_OVERFLOW = 4    /* a device-side capacity check failed */
};

enum { NZ_GAME_TIC_TAC_TOE = 0 };
enum { NZ_ACT_TANH = 0, NZ_ACT_RELU = 1 };
enum { NZ_ARCH_RECURRENT = 0, NZ_ARCH_RESNET = 1, NZ_ARCH_CONVNET = 2 };

/* Search hyper-parameters: exactly the keys the reference's Explorer reads
 * from its search config (Configs/Search/Examples/documentation_search_config.yaml:1-47;
 * Search/Explorer.py:48,74,79-80,105-106,122,202-205). */
typedef struct nz_search_cfg {
  int32_t mcts_simulations;
  int32_t keep_subtree;                 /* must be 1 (Gamer.py:78-79) */
  double pb_c_base;
  double pb_c_init;
  int32_t number_of_softmax_moves;
  int32_t training;                     /* Explorer(search_config, training) */
  double epsilon_softmax_exploration;
  double epsilon_random_exploration;
  double value_factor;
  double root_exploration_fraction;
  double root_dist_alpha;
  double root_dist_beta;
} nz_search_cfg;

/* Game description (the duck-typed Game surface, Games/Game.py). */
typedef struct nz_game_desc {
  int32_t game;                         /* NZ_GAME_* */
  int32_t negate_player;                /* Q is negated iff parent.to_play == this (Explorer.py:124) */
} nz_game_desc;

/* The policy/value networks of the reference (square convs; hexagonal ones for nz_boardnet_*), all with the
 * "conv" policy head and the "reduce" value head (blocks.py:46-92,130-170):
 *   NZ_ARCH_RECURRENT  RecurrentNet(in_channels, policy_channels, num_filters=width, num_blocks,
 *                      recall, value_activation)   (Architectures/RecurrentNet.py:18-99)
 *   NZ_ARCH_RESNET     ResNet(in_channels, policy_channels, num_filters=width, num_blocks,
 *                      batch_norm=False, value_activation)     (Architectures/ResNet.py:13-70)
 *   NZ_ARCH_CONVNET    ConvNet(in_channels, policy_channels, kernel_size, num_filters=width,
 *                      num_layers=num_blocks)  -- ELU trunk          (Architectures/ConvNet.py:12-57)
 * Weights are passed in the model's state_dict order. */
typedef struct nz_net_desc {
  int32_t in_channels;
  int32_t policy_channels;
  int32_t width;
  int32_t num_blocks;                   /* residual blocks; ConvNet: num_layers */
  int32_t recall;                       /* RecurrentNet only */
  int32_t value_activation;             /* NZ_ACT_* */
  int32_t arch;                         /* NZ_ARCH_* */
  int32_t kernel_size;                  /* ConvNet trunk: 1 or 3; others: 3.  With hex: the hexagdly size, 1 */
  int32_t hex;                          /* 1: every conv is hexagdly.Conv2d(kernel_size=1): centre + 6 neighbours on a
                                           grid whose odd columns sit half a cell lower; each conv then has TWO weight
                                           tensors, kernel0 [out][in][3][1] and kernel1 [out][in][2][2].  nz_boardnet_*
                                           only; restated from the hexagdly documentation, parity unpinned (the package
                                           is not installed here).  nz_engine_set_weights rejects it. */
} nz_net_desc;

/* Fixed per-engine sizes, for sizing the caller's export buffers. */
typedef struct nz_dims {
  int32_t n_games;                      /* games per self-play round */
  int32_t n_slots;                      /* games in flight at once */
  int32_t num_actions;                  /* A */
  int32_t max_moves;                    /* T */
  int32_t state_channels, rows, cols;   /* C, H, W */
  int32_t node_capacity;                /* tree arena nodes per game */
} nz_dims;

const char* nz_version(void);
/* Message of the last failure on `e` (or of the last failed nz_engine_create when e == NULL). */
const char* nz_last_error(const nz_engine* e);

/* ---- engine life cycle ---------------------------------------------------
 * Replaces: Gamer.__init__ (Training/Gamer.py:20-37), one per actor, and the
 * per-game `game_class(*game_args)` / `Node(0)` set-up (Gamer.py:52,59). */
nz_status nz_engine_create(nz_engine** out, const nz_search_cfg* cfg, const nz_game_desc* game,
                           int32_t n_games, int32_t device);
/* As nz_engine_create, with the concurrency separate from the round size: a
 * round of n_games games is played on n_slots (<= n_games) concurrent trees; a
 * slot whose game ends takes the next unplayed game, as the reference's
 * ActorPool of num_actors Gamers does for num_games_per_step games
 * (Training/AlphaZero.py:525-577).  nz_engine_create is n_slots == n_games. */
nz_status nz_engine_create_ex(nz_engine** out, const nz_search_cfg* cfg, const nz_game_desc* game,
                              int32_t n_slots, int32_t n_games, int32_t device);
void nz_engine_destroy(nz_engine* e);
nz_status nz_engine_dims(const nz_engine* e, nz_dims* out);

/* Hand the network to the engine.  Replaces `shared_storage.get` +
 * `network_copy.check_devices()` (Gamer.py:40,61-62) and selects what
 * Network_Manager.inference (Neural_Networks/Network_Manager.py:46-64) computes.
 * `weights[i]` are float32 tensors in the reference's state_dict order and
 * [C_out][C_in][3][3] layout (host or device memory); they are repacked for the
 * MFMA kernel and copied, so the caller may free them afterwards.
 * Accepted shapes (anything else: NZ_ERR_ARG and a message): in_channels 2, policy_channels 1, no hex; width a multiple
 * of 4 in (0, 64]; num_blocks >= 0; recurrent_iterations >= 0 (0: the projection conv and the heads; read for
 * NZ_ARCH_RECURRENT only); kernel_size 1 or 3 for the ConvNet trunk only (the heads and the other trunks are 3x3;
 * a 1x1 tensor is [C_out][C_in][1][1]); as many layers as fit one fused launch.  The three routes that run the network -- nz_net_forward, nz_net_forward_packed and
 * nz_engine_play's kernel -- are pinned over these shapes to a float64 reference within 1e-5 and to each other bit for
 * bit by tests/test_gpu_tttnet_edges.py (cases: tests/tttnet_cases.py: widths 4 to 64, 0 to 3 blocks, 0 to 5
 * iterations, recall on and off, both value activations, k = 1 and 3). */
nz_status nz_engine_set_weights(nz_engine* e, const nz_net_desc* net, const float* const* weights,
                                int32_t n_tensors, int32_t recurrent_iterations);

/* Test hook: evaluate leaves by table look-up instead of the network.
 * table[code][0..8] = post-softmax probabilities, table[code][9] = value,
 * code = sum(cell[a] * 3^a); 19683 rows, host or device memory.  Same meaning
 * as a cache hit in Explorer.evaluate (Explorer.py:146-149). */
nz_status nz_engine_set_table(nz_engine* e, const float* table, int32_t n_rows);

/* New batch of games: every game back to the initial position with an
 * unexpanded root (Gamer.py:52-59). */
nz_status nz_engine_reset(nz_engine* e, void* stream);

/* nz_engine_reset, then every game's position becomes boards_host[g] (uint32 [n_games], host memory; copied before the
 * call returns): the engine's own bitboard word, player-one stones in bits 0-8, player-two stones in bits 16-24.
 * A position is playable when no other bit is set, the two stone sets are disjoint, stones(p1) - stones(p2) is 0 or
 * 1, neither side has a line and at least one cell is empty; how it arose is not checked.  The search starts from a
 * fresh root (MctsAgent.new_game, then choose_action on a game stepped to the position), the player to move is the
 * one the stone count gives, and the engine's records count from the position: record 0 is the first decision made
 * there, lengths the plies played since.  Evaluation engines on the lock-step route only.  Refused before any launch,
 * the engine untouched: NZ_ERR_ARG for a NULL argument, a training engine, or a board that is not playable (the
 * message names the index of the first one and the condition); NZ_ERR_STATE for n_slots != n_games.
 * nz_engine_reset afterwards returns the engine to the empty board: nothing of the positions survives. */
nz_status nz_engine_reset_to(nz_engine* e, const uint32_t* boards_host, void* stream);

/* Children of each game's current root, 0 for an unexpanded root or a finished
 * game: the number of gamma draws add_exploration_noise will take
 * (Explorer.py:201-210).  dev int32[G]. */
nz_status nz_engine_root_children(nz_engine* e, int32_t* n_children_dev, void* stream);

/* One move for every live game: Explorer.run_mcts (Explorer.py:40-67:
 * root noise, mcts_simulations x {select, evaluate/expand, backup},
 * select_action) followed by game.step, store_search_statistics and re-rooting
 * (Gamer.py:65-79).
 *   noise_dev    double[G][A]: gamma draws for the root's children in child
 *                order (first n_children entries of a row are used); may be
 *                NULL when training == 0.
 *   uniforms_dev double[G][3]: epsilon_softmax, epsilon_random and the uniform
 *                np.random.choice consumes (Explorer.py:77-78,89,199); may be
 *                NULL when training == 0. */
nz_status nz_engine_move(nz_engine* e, const double* noise_dev, const double* uniforms_dev,
                         void* stream);

/* The two halves of nz_engine_move, for evaluation matches (Testing/Tester.py:46-121 with
 * Testing/Agents/Generic/MctsAgent.py:28-39):
 *   nz_engine_search  root noise (training only) + the simulations, no action yet;
 *   nz_engine_apply   select the action -- the search's own choice when actions_dev is NULL
 *                     (MctsAgent.choose_action), else actions_dev[g] (the opponent's move in
 *                     MctsAgent.update_subtree) -- then step, record and re-root;
 *   nz_engine_last_actions  the action each game took at its latest move (dev int32[G], -1 if none).
 * An agent that keeps its subtree searches on the opponent's turn too, so a match between two
 * MCTS agents is two engines that both search every ply and both apply the mover's action. */
nz_status nz_engine_search(nz_engine* e, const double* noise_dev, void* stream);
nz_status nz_engine_apply(nz_engine* e, const int32_t* actions_dev, const double* uniforms_dev, void* stream);
nz_status nz_engine_last_actions(nz_engine* e, int32_t* actions_dev, void* stream);

/* 1 for every game that is not yet terminal, else 0.  dev int32[G]. */
nz_status nz_engine_alive(nz_engine* e, int32_t* alive_dev, void* stream);

/* Number of games not yet terminal.  Synchronises `stream`. */
nz_status nz_engine_live_games(nz_engine* e, int32_t* n_live_host, void* stream);

/* Whole games with the engine's own host random streams: game g uses a private
 * legacy MT19937 stream seeded base_seed + g, consumed in the reference's order
 * (SURVEY.md appendix A rules 13-17).  Resets, then plays until every game is
 * terminal (Gamer.play_game, Gamer.py:39-97, for G games).  Synchronises. */
nz_status nz_engine_play(nz_engine* e, uint64_t base_seed, void* stream);
/* As nz_engine_play; with have_next the random numbers of the round that will be played next (seeds
 * next_base_seed + g) are drawn on the host threads while this round's kernel runs, and the next call with that
 * base seed uses them (any other call draws afresh: results never depend on the hint). */
nz_status nz_engine_play_next(nz_engine* e, uint64_t base_seed, int32_t have_next, uint64_t next_base_seed, void* stream);

/* Same games, same results, by the lock-step route: one kernel sequence per move
 * with a host round trip in between (the route nz_engine_move exposes).
 * nz_engine_play runs the persistent self-play kernel instead and falls back to
 * this route for the rare game whose pre-drawn randomness does not fit. */
nz_status nz_engine_play_lockstep(nz_engine* e, uint64_t base_seed, void* stream);
/* Games nz_engine_play had to replay by the lock-step route since creation. */
nz_status nz_engine_desync_count(const nz_engine* e, int64_t* count_host);

/* Results of the batch, the data ReplayBuffer.save_game reads from a game
 * (Training/ReplayBuffer.py:24-36) plus the per-move statistics Gamer reports
 * (Gamer.py:42-50,81-92).  Any pointer may be NULL.  T = max_moves.
 *   states    float [G][T][C][H][W]  game.state_history (zeros past the end)
 *   visits    int32 [G][T][A]        root child visit counts by action
 *                                    (child_policy = visits / sum, tic_tac_toe.py:177-182)
 *   actions   int32 [G][T]           chosen action, -1 past the end
 *   lengths   int32 [G]              game.length
 *   outcomes  int32 [G]              game.terminal_value
 *   tree_size int32 [G][T]           root.visit_count after the search (Gamer.py:71)
 *   n_children int32[G][T]           root.num_children()             (Gamer.py:72)
 *   bias      double[G][T]           final_root_bias                 (Explorer.py:63)
 */
nz_status nz_engine_export(nz_engine* e, float* states, int32_t* visits, int32_t* actions,
                           int32_t* lengths, int32_t* outcomes, int32_t* tree_size,
                           int32_t* n_children, double* bias, void* stream);

/* Parity trace of the root's children after each search, by action index:
 * prior (after noise), value_sum; plus root value_sum.  dev double[G][T][A],
 * double[G][T][A], double[G][T].  Any pointer may be NULL. */
nz_status nz_engine_export_trace(nz_engine* e, double* child_prior, double* child_value_sum,
                                 double* root_value_sum, void* stream);

/* Work counters since the last reset, summed over games: simulations and
 * node expansions (= network evaluations, Explorer.py:144-181).  Synchronises. */
nz_status nz_engine_counters(nz_engine* e, int64_t* simulations_host, int64_t* expansions_host,
                             void* stream);
/* As above plus the select work done: out[0] simulations, out[1] expansions,
 * out[2] internal nodes whose children were scored (descent levels), out[3]
 * children scored.  Writes exactly FOUR values. */
nz_status nz_engine_counters_ex(nz_engine* e, int64_t* out4_host, void* stream);
/* The first n_out (1..5) of: the four above, then out[4] nodes created by
 * expansions.  Used to price the tree phase's algorithmic bytes (SURVEY.md
 * section 8d).  The caller states its array's length, so later additions never
 * write past an older caller's array. */
nz_status nz_engine_counters_n(nz_engine* e, int64_t* out_host, int32_t n_out, void* stream);

/* Algorithmic FLOPs of one network evaluation (one position): sum over convs of
 * 2 * C_out * C_in * 49, i.e. only the taps that fall inside the 3x3 board. */
nz_status nz_engine_net_flops(const nz_engine* e, double* flops_host);
/* What the matrix cores execute per position for it: the fused kernel forms each float32
 * product from six bf16 MFMA terms on exact three-way splits (bf16_flops, including the
 * zero-padded channels of 32-channel K groups) and uses float32 MFMAs for the raw input
 * planes (f32_flops). */
nz_status nz_engine_net_matrix_flops(const nz_engine* e, double* bf16_flops_host, double* f32_flops_host);

/* The job lists the fused network kernel runs for `net` (what nz_engine_set_weights compiles; host only, no device is
 * touched): one row of NZ_NET_JOB_FIELDS int32 per job -- wave, stage, output-cell group, the group's cells (bit o =
 * cell o), K groups, first source slot (-1: split over a buffer and the strip), source buffer, destination (0, 1:
 * activation buffers, 2: policy logits, 3: value, 4: the strip), residual buffer or -1, activation (0 none, 1 relu,
 * 2 tanh, 3 elu), destination tile, 1 if the input planes are read, 1 if the job's epilogue is issued cell by cell
 * inside its K loop.  Writes at most max_jobs rows and sets *n_jobs to the number of jobs. */
#define NZ_NET_JOB_FIELDS 13
nz_status nz_net_program(const nz_net_desc* net, int32_t recurrent_iterations, int32_t* jobs, int32_t max_jobs,
                         int32_t* n_jobs);
/* The order in which wave `wave` runs jobs in a pass it steals (it runs, stage by stage, its own jobs and then those of
 * wave `wave` ^ 4, which sits the pass out; host only): one row of NZ_NET_STEAL_FIELDS int32 per job, barrier-only jobs
 * included -- the list's wave, index in that list, stage, output-cell group (7: no work), K groups, dword offset of
 * the job's weights, that of the weights the job streams in behind its own (-1: none), destination, destination tile,
 * 1 if a stage of that list ends with the job, the stage's simulation budget.  *first_w: the weights in the ring when
 * the pass starts (-1: none).
 * This is the CONCATENATED order: what the kernel walks when NZ_BURST_WHOLE_TILE=0 is set, and what the whole-tile jobs
 * of nz_net_solo_program are made of; it does not depend on that switch. */
#define NZ_NET_STEAL_FIELDS 11
nz_status nz_net_steal_order(const nz_net_desc* net, int32_t recurrent_iterations, int32_t wave, int32_t* rows,
                             int32_t max_rows, int32_t* n_rows, int32_t* first_w);
/* The list wave `wave` actually walks in a pass it steals (host only): the concatenated order above, except that where
 * the two waves' jobs of a stage are the two cell halves (groups 5 and 6) of one tile of one conv into an activation
 * buffer -- same weights, K groups, source, first slot, destination, tile, residual, activation and input-plane step
 * -- ONE job of group 0 (all nine cells) stands for both, unless NZ_BURST_WHOLE_TILE=0 is set in the environment.  One
 * row of NZ_NET_SOLO_FIELDS int32 per job, barrier-only jobs (group 7) included: the NZ_NET_JOB_FIELDS fields of
 * nz_net_program (`wave` is the walking wave), then the dword offset of the job's weights, that of the weights it
 * streams in behind its own (-1: none), and 1 if the workgroup barrier of a stage follows the job.  *first_w as above. */
#define NZ_NET_SOLO_FIELDS (NZ_NET_JOB_FIELDS + 3)
nz_status nz_net_solo_program(const nz_net_desc* net, int32_t recurrent_iterations, int32_t wave, int32_t* jobs,
                              int32_t max_jobs, int32_t* n_jobs, int32_t* first_w);
/* last conv tap (0..8, row-major over (dy, dx) in -1..1) that reaches output cell `cell` of the 3x3 board; -1: no such cell */
int32_t nz_net_final_tap(int32_t cell);

/* ---- stand-alone operators (same kernels, callable by themselves) ---------
 * Network_Manager.inference for a batch (Network_Manager.py:46-64):
 * states float[B][C][3][3] -> logits float[B][P*9], value float[B]; and the
 * softmax Explorer.evaluate applies (Explorer.py:159) -> probs float[B][P*9]
 * (may be NULL). */
nz_status nz_net_forward(nz_engine* e, const float* states_dev, int32_t batch, float* logits_dev,
                         float* value_dev, float* probs_dev, void* stream);

/* ---- the packed network pass: a pass sized for a few positions per workgroup ----
 * The persistent kernel gives a workgroup ceil(n_slots / CUs) games; with P <= NZ_NET_PACKED_MAX of them the 16 columns
 * of its matrix instructions can be (position, cell) pairs instead of positions: ceil(9 P / 16) column tiles, nine
 * six-MFMA chains each per K group and output tile, where the 16-position tile costs 49.  The outputs are bit for bit
 * those of the 16-position tile.  NZ_NET_PACKED in the environment at nz_engine_create: 0 = never, N = engines with at
 * most N games per workgroup, unset = the measured rule. */
#define NZ_NET_PACKED_MAX 8
/* nz_net_forward's outputs from a kernel of one workgroup per `positions_per_pass` (1 .. NZ_NET_PACKED_MAX) positions
 * that runs the packed pass. */
nz_status nz_net_forward_packed(nz_engine* e, const float* states_dev, int32_t batch, int32_t positions_per_pass,
                                float* logits_dev, float* value_dev, float* probs_dev, void* stream);
/* Positions a network pass of nz_engine_play's kernel is sized for: 16 (the full tile), or the engine's games per
 * workgroup when it takes the packed pass. */
nz_status nz_engine_positions_per_pass(const nz_engine* e, int32_t* out);
/* The column map of the packed pass for P positions (host only): *n_tiles = T = ceil(9 P / 16) column tiles, and for
 * column j of tile t, at index i = 16 t + j: col_pos[i] and col_cell[i] (-1, -1: a dead column) and tap_src[9 i + tap],
 * the cell of the same position whose activations the column reads for `tap` (tap = 3 (dy + 1) + (dx + 1) as for
 * nz_net_final_tap; -1: off the board or dead, a zero fragment).  Arrays of max_cols entries (9 max_cols for tap_src);
 * NZ_ERR_ARG when 16 T exceeds max_cols. */
nz_status nz_net_packed_columns(int32_t P, int32_t* col_pos, int32_t* col_cell, int32_t* tap_src, int32_t max_cols,
                                int32_t* n_tiles);
/* The job lists of the packed pass for `net` and P positions (host only): one row of NZ_NET_PACKED_JOB_FIELDS int32 per
 * job, barrier-only jobs included -- wave, stage, conv tensor (state_dict order; -1: barrier only), output tile, first
 * column tile, column tiles, K groups, source area, destination (0 .. 3: areas, 8: policy logits, 9: value), residual
 * area or -1, activation (0 none, 1 relu, 2 tanh, 3 elu), 1 if the input planes are read, 1 if the workgroup barrier
 * of a stage follows the job, output tiles of the conv.  Writes at most max_jobs rows, sets *n_jobs to their number. */
#define NZ_NET_PACKED_JOB_FIELDS 14
nz_status nz_net_packed_program(const nz_net_desc* net, int32_t recurrent_iterations, int32_t P, int32_t* jobs,
                                int32_t max_jobs, int32_t* n_jobs);

/* For each row of nz_net_program, in the same order, the conv tensor (state_dict order) the job applies (host only):
 * with the row's stage, destination, tile and cells this names the layer that wrote any stored activation. */
nz_status nz_net_program_convs(const nz_net_desc* net, int32_t recurrent_iterations, int32_t* conv_of_job, int32_t max_jobs,
                               int32_t* n_jobs);

/* ---- the plain-bf16 mode of the Tic-Tac-Toe network (opt-in; the board nets' rule, nz_boardnet_precision below) ----
 * NZ_PREC_FLOAT32, the default, is the arithmetic above.  NZ_PREC_BF16: weights and input-plane weights rounded once on
 * the host (to nearest even), raw input planes rounded where the kernel reads them, every stored activation rounded
 * once in the epilogue that makes it; a conv accumulates in float32 with ONE bf16 MFMA per (input cell, tap) pair and K
 * group in the float32 mode's order, adds the residual as the stored bf16 value, applies the float32 mode's activation
 * functions and stores one bf16.  Logits, the value's per-cell staging, tanh(mean) and the softmax stay float32.  Job
 * lists and LDS layout are unchanged; the weight stream has no piece dimension and is the only one built in the mode.
 * `mode`: NZ_PREC_FLOAT32 / NZ_PREC_BF16, -1 only reads; anything else is NZ_ERR_ARG.  Setting a DIFFERENT mode drops
 * the engine's weights (nz_net_forward, nz_engine_play* and the other network routes return NZ_ERR_STATE until the next
 * nz_engine_set_weights; a table set with nz_engine_set_table stays) and re-derives the pass choice: the mode exists
 * for the 16-column pass on a wave's own job list only, so a bf16 engine plays with burst_under_net off and never
 * takes the packed pass, whatever NZ_BURST_UNDER_NET / NZ_NET_PACKED say (both are results-neutral: this costs speed
 * at small engines, not games); nz_engine_positions_per_pass reports 16, nz_net_forward_packed and
 * nz_net_forward_stamps return NZ_ERR_STATE.  Nothing falls back to float32.  The persistent kernel, the lock-step
 * route, nz_engine_move / _search, nz_engine_match_play*, nz_engine_policy_actions and nz_net_forward all follow the
 * mode; nz_engine_net_matrix_flops reports one bf16 term per product in it.  (NZ_PREC_*: declared with
 * nz_boardnet_precision; the values are 0 and 1.) */
nz_status nz_engine_precision(nz_engine* e, int32_t mode, int32_t* current);
/* The mode's weight stream of one conv tensor w [cout][cin][k][k] (k 1 or 3; host only, as nz_engine_set_weights packs
 * it): *n_main words [output tile][K group of 32][tap][lane][4], a word two rounded bf16 of neighbouring input
 * channels < cin_main, then *n_extra words, the float32 bits of the rounded input-plane weights [output tile][tap][lane]
 * (channels cin_main .. cin - 1; none when cin == cin_main).  Writes at most max_words words. */
nz_status nz_net_bf16_stream(const float* w, int32_t cout, int32_t cin, int32_t cin_main, int32_t k, uint32_t* words,
                             int64_t max_words, int64_t* n_main, int64_t* n_extra);
/* The test hook of the mode (NZ_ERR_STATE in float32 mode): nz_net_forward's outputs and, per position, what the device
 * itself held, widened to float32.  With R = 16 * ceil(batch / 16) rows (all 16 of every tile, live or not):
 *   planes_dev float[R][9 cells][4]      the rounded input planes (planes 2, 3: zero)
 *   acts_dev   float[max_stages][R][NZ_NET_DUMP_ROW]   after stage s (nz_net_program's stage index): piece plane 0 of
 *              activation buffer 0, of buffer 1 ([cell][64 channels] each), then of the strip ([cell][16 channels]);
 *              stages past max_stages are not written
 *   vcells_dev float[R][9]               the value head's per-cell staging before the mean
 * *n_stages (may be NULL): the program's stages.  It runs a kernel instantiation of its own with one more barrier
 * after each stage; the plain bf16 kernel carries none of it. */
#define NZ_NET_DUMP_ROW (2 * 9 * 64 + 9 * 16)
nz_status nz_net_forward_dump(nz_engine* e, const float* states_dev, int32_t batch, float* logits_dev, float* value_dev,
                              float* probs_dev, float* planes_dev, float* acts_dev, int32_t max_stages, float* vcells_dev,
                              int32_t* n_stages, void* stream);

/* Diagnostic build of the network kernel: mean shader-clock ticks wave 0 of a
 * workgroup spends in [0] the K-group loops (LDS reads + MFMA), [1] the
 * input-plane step, [2] the epilogues, [3] at the stage barriers.  Synchronises. */
nz_status nz_net_forward_stamps(nz_engine* e, const float* states_dev, int32_t batch, float* logits_dev,
                                float* value_dev, double* ticks4_host);

/* Timing of the engine's own kernels, measured with HIP events on the stream
 * the kernels run on.  Enable, run, then read: total milliseconds and launch
 * count per kernel class (0 = search: the persistent self-play kernel or the lock-step
 * advance kernel, 1 = stand-alone network kernel, 2 = move/noise/reset/export). */
nz_status nz_engine_profile(nz_engine* e, int32_t enable);
nz_status nz_engine_profile_read(nz_engine* e, double* ms_host /*[3]*/, int64_t* launches_host /*[3]*/,
                                 int64_t* net_positions_host);

/* Diagnostic build of the persistent kernel: with `enable` the next
 * nz_engine_play runs the stamped variant (shader-clock ticks per phase).  If
 * out4_host is not NULL it first receives the last stamped run's figures:
 * [0] mean tree/net cycles per workgroup, [1] share of ticks in the tree phase,
 * [2] share in the network phase, [3] mean / max workgroup lifetime (how evenly
 * the workgroups finish), [4] shader-clock ticks per network phase, [5] per tree
 * phase, [6] ticks of the longest-lived workgroup, [7] workgroups, [8] wave 0's
 * ticks per cycle in end-of-move bookkeeping, [9] simulations of the slowest row per
 * cycle, [10] network passes per workgroup during which a wave sat out, [11]
 * simulations per workgroup run under network passes.  Run times of the stamped
 * build are not quoted. */
nz_status nz_engine_phase_stamps(nz_engine* e, int32_t enable, double* out12_host);

/* ---- SCS rules as batch operators ------------------------------------------
 * Device-side state transition, legal-move mask and state image of the SCS hex
 * war-game (Games/SCS/SCS_Game.py: step :375-391, possible_actions :395-484,
 * update_game_env :687-831, resolve_combat :997-1044, generate_state :1348-1505),
 * one independent game per batch row.  The search is not built on them yet; they
 * exist so that the rules can be checked against the oracle step by step.
 * A game is described by plain arrays (what load_game_from_config, :1570-1779,
 * reads from the YAML file, "Detailed" map / victory points only):
 *   terrain  float[rows*cols][3]  attack modifier, defense modifier, movement cost
 *   vp       int32[n_vp[0]+n_vp[1]][2]  (row, col), player one's points first
 *   units    int32[n_units][5]  player (0/1), arrival turn, attack, defense, movement;
 *            in schedule order: player one's turns 0..T, then player two's
 *   arrival  uint8[n_units][rows*cols]  1 where the unit may be placed            */
typedef struct nz_scs nz_scs;
typedef struct nz_scs_desc {
  int32_t rows, cols, turns, stacking;
  const float* terrain;
  int32_t n_vp[2];
  const int32_t* vp;
  int32_t n_units;
  const int32_t* units;
  const uint8_t* arrival;
} nz_scs_desc;
nz_status nz_scs_create(nz_scs** out, const nz_scs_desc* desc, int32_t n_games, int32_t device);
void nz_scs_destroy(nz_scs* h);
const char* nz_scs_last_error(const nz_scs* h);
nz_status nz_scs_dims(const nz_scs* h, int32_t* planes, int32_t* rows, int32_t* cols, int32_t* channels);
nz_status nz_scs_reset(nz_scs* h, void* stream);
/* actions_dev int32[G]: flat action index (plane, row, col) or -1 to leave the game as it is */
nz_status nz_scs_step(nz_scs* h, const int32_t* actions_dev, void* stream);
/* mask_dev int8[G][planes*rows*cols]; all zero for a finished game */
nz_status nz_scs_legal_mask(nz_scs* h, int8_t* mask_dev, void* stream);
/* image_dev float[G][channels][rows][cols] = generate_state() */
nz_status nz_scs_state_image(nz_scs* h, float* image_dev, void* stream);
/* status_dev int32[G][7]: player, sub_phase, stage, turn, terminal, terminal_value, length */
nz_status nz_scs_status(nz_scs* h, int32_t* status_dev, void* stream);

/* ---- MCTS self-play on SCS, lock-step, evaluations supplied by the caller -----
 * Explorer.run_mcts / Gamer.play_game for G SCS games with the tree, the rules and the
 * legal-move masks on the device; the network stays outside: nz_scs_search_select hands
 * out the state images of the leaves that need an evaluation (what Explorer.evaluate
 * passes to Network_Manager.inference, Explorer.py:145-158) and nz_scs_search_expand
 * takes (softmax probabilities, value) back (Explorer.py:159-181).  Any PyTorch model
 * can therefore drive the search (hex or square convs) until the fused kernel covers
 * SCS boards.  One move for all live games:
 *   root_children -> host draws gamma noise -> begin_move(noise [G][C], C = nz_scs_search_limits' max_children)
 *   repeat: select(images [G][C][R][Cc], leaf_game [G], &n) ; if n == 0 break ;
 *           evaluate images[0..n) ; expand(probs [n][A], value [n])
 *   end_move(uniforms [G][3])
 * The kernels OR their checks into one device word; the calls that synchronise (select, end_move, apply, the play
 * and match loops) return NZ_ERR_OVERFLOW with the word and its meanings in the message while any bit is set, until the
 * next reset: 1 arena full, 2 visit table / path too short, 4 a move ended before its search (simulations left or a leaf
 * pending), 8 forced action not legal, 16 more legal actions than the bound computed at create, 32 game longer than that
 * bound, 64 RESERVED (the match check reports in the same word that its two engines no longer hold the same game),
 * 128 the position has no legal action although the game is not over: a searched root (no simulation left, no leaf
 * pending) without a child.  The reference raises there (IndexError in max_action); the move's simulations have run (each
 * evaluated the root), no action is played for that game, the other games of the call complete their move, and the
 * message names the first such game and its decision number.  Inside the tree such a node is evaluated at every visit,
 * gets no children and its value is backed up, as the reference does.
 * nodes_per_game sizes each game's tree arena: two halves; at every re-root the new root's subtree is copied
 * into the other half (the rest of the tree is dropped), so a half must hold the kept subtree plus one move's
 * expansions (32 bytes per node; a full half is reported as NZ_ERR_OVERFLOW).  nodes_per_game <= 0: the default,
 * 2 x (1 + simulations x 2.5 x the children bound). */
typedef struct nz_scs_search nz_scs_search;
nz_status nz_scs_search_create(nz_scs_search** out, const nz_scs_desc* desc, const nz_search_cfg* cfg,
                               int32_t n_games, int32_t nodes_per_game, int32_t device);
void nz_scs_search_destroy(nz_scs_search* h);
const char* nz_scs_search_last_error(const nz_scs_search* h);
nz_status nz_scs_search_reset(nz_scs_search* h, void* stream);
nz_status nz_scs_search_root_children(nz_scs_search* h, int32_t* n_children_dev, void* stream);
nz_status nz_scs_search_begin_move(nz_scs_search* h, const double* noise_dev, void* stream);
/* Synchronises; *n_leaves_host = number of leaves queued (0: every game's search is complete). */
nz_status nz_scs_search_select(nz_scs_search* h, float* images_dev, int32_t* leaf_game_dev,
                               int32_t* n_leaves_host, void* stream);
nz_status nz_scs_search_expand(nz_scs_search* h, const float* probs_dev, const float* value_dev, void* stream);
nz_status nz_scs_search_end_move(nz_scs_search* h, const double* uniforms_dev, void* stream);
/* Test hook: the legal masks stored with the pending leaves, masks_dev uint32[G][*words_host] (action a: bit a & 31 of
 * word a >> 5; masks_dev NULL: the row length alone).  A row is meaningful between select and expand, for the games of
 * leaf_game; an all-zero row is a live position without a legal action (its expansion makes no child). */
nz_status nz_scs_search_leaf_masks(nz_scs_search* h, uint32_t* masks_dev, int32_t* words_host, void* stream);
/* status_dev int32[G][7] as nz_scs_status */
nz_status nz_scs_search_status(nz_scs_search* h, int32_t* status_dev, void* stream);
/* Per move m < M of game g (dev pointers, any may be NULL; M = max_moves, C = max_children of
 * nz_scs_search_limits): actions int32[G][M] (-1 past the end), tree_size, n_children int32[G][M], bias,
 * root_value_sum double[G][M]; the root's children in child order: child_action, child_visit int32[G][M][C],
 * child_prior, child_value_sum double[G][M][C].  counters_host int64[2]: simulations, expansions. */
nz_status nz_scs_search_export(nz_scs_search* h, int32_t* actions, int32_t* tree_size, int32_t* n_children,
                               double* bias, double* root_value_sum, int32_t* child_action,
                               int32_t* child_visit, double* child_prior, double* child_value_sum,
                               int64_t* counters_host, void* stream);

/* ---- policy/value network on boards of any size (SCS maps) -------------------
 * The square-conv (hex=False) RecurrentNet / ResNet / ConvNet of the reference
 * (Neural_Networks/Architectures/RecurrentNet.py:18-99, ResNet.py:13-70, ConvNet.py:12-57,
 * blocks.py) on rows x cols boards, evaluated on a batch of state images: what
 * Network_Manager.inference (Network_Manager.py:46-64) plus the softmax of
 * Explorer.evaluate (Explorer.py:158-162) compute for one position, for n positions.
 * Every convolution is an implicit-GEMM FP32 MFMA kernel; activations stay on the device.
 *   images_dev  float[n][in_channels][rows][cols]   (Game.generate_network_input)
 *   logits_dev  float[n][policy_channels*rows*cols] raw policy logits, may be NULL
 *   probs_dev   float[n][policy_channels*rows*cols] softmax over ALL logits, may be NULL
 *   value_dev   float[n]
 *   n_dev       optional device int32: the live batch size (<= n) when the host does not
 *               know it yet (the leaf count of a simulation wave); NULL = n.  Outputs of the
 *               positions from *n_dev on are not written; *n_dev == 0 writes nothing at all
 *               and returns NZ_OK (as n == 0 does, without a launch).
 * Shapes (pinned by tests/test_gpu_boardnet_edges.py against a float64 reference): any positive
 * rows and cols (a board may be one cell wide or high), any positive width, in_channels and
 * policy_channels (none has to be a multiple of 16), num_blocks >= 0, kernel_size 1 or 3
 * (ConvNet trunk; the heads are 3x3), 0 <= n <= max_batch, RecurrentNet iterations >= 1.
 * Anything else is refused with NZ_ERR_ARG and a message in nz_boardnet_last_error (of the
 * handle, or of NULL where there is no handle). */
typedef struct nz_boardnet nz_boardnet;
nz_status nz_boardnet_create(nz_boardnet** out, const nz_net_desc* net, int32_t rows, int32_t cols,
                             int32_t max_batch, int32_t device);
void nz_boardnet_destroy(nz_boardnet* h);
const char* nz_boardnet_last_error(const nz_boardnet* h);
/* weights: the state_dict tensors in order (float32, device or host), as nz_engine_set_weights */
nz_status nz_boardnet_set_weights(nz_boardnet* h, const float* const* weights, int32_t n_weights,
                                  int32_t recurrent_iterations);
nz_status nz_boardnet_forward(nz_boardnet* h, const float* images_dev, int32_t n, const int32_t* n_dev,
                              float* logits_dev, float* probs_dev, float* value_dev, void* stream);
/* The same without the layout conversion: the network's own input buffer is rows of `row_stride` floats, channels
 * contiguous, row = ((position / 16) * rows*cols + cell) * 16 + position % 16.  A producer (the SCS search kernel)
 * writes the positions' planes there directly, then calls nz_boardnet_forward_rows.  What the caller owes: channels
 * 0 .. in_channels - 1 of every cell of the n (or *n_dev) live positions, written on `stream` or ordered before it.
 * The channels from in_channels to row_stride are zero after nz_boardnet_create and after every nz_boardnet_forward
 * and are best left alone; they meet zero weights, so any FINITE value there leaves the outputs unchanged, a NaN or
 * an infinity does not.  Rows of positions past the live ones (up to max_batch rounded up to 16) may hold any finite
 * values, stale planes of an earlier, larger batch included: no live position's output depends on them.  The buffer belongs
 * to the handle (max_batch rounded up to 16 positions) and is overwritten by nz_boardnet_forward. */
nz_status nz_boardnet_input_rows(nz_boardnet* h, float** rows_dev, int32_t* row_stride);
nz_status nz_boardnet_forward_rows(nz_boardnet* h, int32_t n, const int32_t* n_dev, float* logits_dev, float* probs_dev,
                                   float* value_dev, void* stream);
/* algorithmic FLOPs of one position (taps that fall off the board are not counted) */
int64_t nz_boardnet_flops(const nz_boardnet* h);
/* Narrow nets on small boards run all layers, the softmax and the value in ONE launch with the activations in LDS
 * (when a workgroup's share of max_batch fits; same floats as the per-layer kernels).  enable: 1 / 0 switch it on /
 * off (the A/B of the parity test), -1 leaves it; *available (may be NULL): whether the one-launch form was built. */
nz_status nz_boardnet_fused(nz_boardnet* h, int32_t enable, int32_t* available);
nz_status nz_boardnet_dims(const nz_boardnet* h, int32_t* in_channels, int32_t* policy_channels, int32_t* rows,
                           int32_t* cols, int32_t* max_batch);
/* The arithmetic of the one-launch BF16 program (fused16_net_kernel) and of the per-wavefront form of the persistent SCS
 * kernel.  NZ_PREC_FLOAT32, the default, is the arithmetic described above: every float32 product from six bf16 MFMA terms
 * on exact three-way splits, 1e-5 from the reference.  NZ_PREC_BF16 is opt-in plain bf16 for self-play that wants
 * throughput over parity: weights, input planes and every stored activation are ONE bf16 (round to nearest even), a
 * product is one v_mfma_f32_16x16x32_bf16 with float32 accumulation, the residual is the stored bf16 value, the logits, the
 * softmax and the value stay float32.  Its outputs are 6e-3 .. 2e-2 from the reference (tests/test_bf16_ref_host.py).
 *   set       NZ_PREC_FLOAT32 / NZ_PREC_BF16; -1 only reads.  Setting a DIFFERENT mode puts the handle back to "no weights
 *             set" (NZ_ERR_STATE from every forward until the next nz_boardnet_set_weights, which builds in the new mode).
 *   *current  (may be NULL) the handle's mode.
 * The bf16 mode exists exactly where a Fused16Program can be built: ConvNet / ResNet, every layer of at most 64 padded
 * channels, a workgroup's share of max_batch in LDS, square or hexagonal.  nz_boardnet_set_weights on any other network in
 * bf16 mode is NZ_ERR_ARG and names the reason (a RecurrentNet, a layer wider than 64, LDS); nothing falls back to
 * float32.  In bf16 mode nz_boardnet_fused(h, 0, ...) is NZ_ERR_STATE (the per-layer kernels are float32), and so is
 * setting the mode while the one-launch form is switched off.
 * An inference cache (nz_scs_search_cache) holds the evaluations of the network and mode it was filled with: after a
 * change of mode empty it, nz_scs_search_cache(h, -1), as after a change of weights. */
enum { NZ_PREC_FLOAT32 = 0, NZ_PREC_BF16 = 1 };
nz_status nz_boardnet_precision(nz_boardnet* h, int32_t set, int32_t* current);
/* Host only, no device needed: the bf16 mode's weight stream of one single-source conv layer as nz_boardnet_set_weights
 * packs it -- [16-channel output tile][tap][32-channel input group][lane 0..63][4 words], a word = the bf16 (round to
 * nearest even) of input channels (32 group + 8 (lane / 16) + 2 word, + 1) for output channel 16 tile + lane % 16, low half
 * first; taps: 3 (dy + 1) + (dx + 1), a 1x1 kernel at tap 4; hexagonal N, centre, S, NW, SW, NE, SE.  w0, w1: host
 * tensors as for set_weights (w1 = kernel1 of a hexagonal conv, else NULL).  Pinned by tests/test_bf16_ref_host.py. */
nz_status nz_boardnet_bf16_stream(const float* w0, const float* w1, int32_t cout, int32_t cin, int32_t kernel_size, int32_t hex,
                                  uint32_t* out, int64_t cap, int64_t* n_words);
/* Test hook of the bf16 mode (NZ_ERR_STATE in float32 mode): nz_boardnet_forward that also copies what every layer
 * stored in LDS to dump_dev, widened to float32.  Section 0 is the rounded input, section 1 + i layer i's output (layers in
 * state_dict order: trunk, policy head, value head); section s is float[n][rows_per_position[s]][channels[s]], the sections
 * back to back.  A bf16 buffer gives rows*cols rows and then its row of zeros (what an off-board tap reads); the float32
 * rows of the logits and of the value plane give rows*cols rows.  Channels: the input's padded to whole 32-channel groups,
 * a layer's the 16 per output tile it stored (its padded output channels included).  nz_boardnet_dump_layout fills the first `cap`
 * entries of the two arrays (either may be NULL) and *n_sections; dump_floats is the size of dump_dev in floats. */
nz_status nz_boardnet_dump_layout(nz_boardnet* h, int32_t* n_sections, int32_t* rows_per_position, int32_t* channels, int32_t cap);
nz_status nz_boardnet_forward_dump(nz_boardnet* h, const float* images_dev, int32_t n, float* dump_dev, int64_t dump_floats,
                                   const int32_t* n_dev, float* logits_dev, float* probs_dev, float* value_dev, void* stream);

/* Gamer.play_game (Training/Gamer.py:52-92) for all G SCS games of `h` to the end, tree, rules,
 * masks AND network on the device: one simulation wave = one [expand + select] kernel followed
 * by nz_boardnet_forward on the wave's leaves, whose count stays in device memory.  The host
 * draws each move's random numbers (game g uses numpy RandomState(seeds_host[g]) in the
 * reference's order) and polls for the end of the move's searches every few waves.
 * Synchronises.  Read the games with nz_scs_search_export / nz_scs_search_status. */
nz_status nz_scs_search_play(nz_scs_search* h, nz_boardnet* net, const uint32_t* seeds_host, void* stream);
/* As nz_scs_search_play, stopping after `max_moves` decisions of every game (<= 0: play to the end): the
 * first moves of a game are exactly those of the full game (Gamer.py:64-79 has no look-ahead), so this
 * bounds a check on a large board / a heavy network without changing what is checked. */
nz_status nz_scs_search_play_moves(nz_scs_search* h, nz_boardnet* net, const uint32_t* seeds_host, int32_t max_moves,
                                   void* stream);

/* A round of n_round >= n_games games over the engine's n_games slots: a slot whose game has ended hands its records to
 * the round's store and starts the round's next game, as a Gamer actor plays its games back to back
 * (Training/Gamer.py:45-98) -- the round ends with its longest game instead of idling the slots of short ones.  Game i
 * is seeded with seeds_host[i] (numpy RandomState(seed), the reference's draw order) whichever slot plays it, so a
 * round's games do not depend on the number of slots.  n_round == n_games is nz_scs_search_play. */
nz_status nz_scs_search_play_round(nz_scs_search* h, nz_boardnet* net, const uint32_t* seeds_host, int64_t n_round,
                                   void* stream);
/* nz_scs_search_export for the last round of more games than slots: every array has n_round rows;
 * status2 [n_round][2] = (length, terminal value).  Device pointers, any may be null. */
nz_status nz_scs_search_export_round(nz_scs_search* h, int32_t* actions, int32_t* tree_size, int32_t* n_children,
                                     double* bias, double* root_value_sum, int32_t* child_action, int32_t* child_visit,
                                     double* child_prior, double* child_value_sum, int32_t* status2,
                                     int64_t* counters_host, void* stream);
/* Diagnostic (library built with -DNZ_SCS_STAMPS, zeros otherwise): shader ticks summed over games and waves since
 * the last reset; out6: expansion, rules copy, scratch clone, descent, leaf mask + image, terminal simulations. */
nz_status nz_scs_search_phase_ticks(nz_scs_search* h, int64_t* out6_host);
/* Evaluation matches on SCS (Testing/Agents/Generic/MctsAgent.py:28-39, Testing/Tester.py:46-121), as
 * nz_engine_search / _apply / _last_actions for Tic-Tac-Toe: after a move's search (begin_move + select / expand until
 * no leaf is left) nz_scs_search_apply plays actions_dev[g] (int32 [G]; NULL or -1: the search's own choice,
 * like nz_scs_search_end_move), steps and re-roots; nz_scs_search_last_actions gives each game's latest action. */
nz_status nz_scs_search_apply(nz_scs_search* h, const int32_t* actions_dev, const double* uniforms_dev, void* stream);
nz_status nz_scs_search_last_actions(nz_scs_search* h, int32_t* actions_dev, void* stream);

/* The reference's optional inference cache (Explorer.py:146-155; Utils/Caches/KeylessCache.py:24-160, DictCache.py:4-85;
 * handed to Gamer.play_game by AlphaZero.py:560-577) for nz_scs_search_play: one keyless hash table in HBM shared by the
 * games of the engine -- a leaf whose state was evaluated before takes (probs, value) from the table instead of the
 * network.  Results-neutral: a position's evaluation does not depend on the batch it was computed in.  The key is the
 * state and, with per-game maps (nz_scs_search_set_games), a digest of the game's map: games on different maps never
 * share an entry, games on equal maps do (the reference hashes the state tensor, which holds the map's planes).
 *   max_entries > 0: (re)allocate an empty table of the largest power of two <= max_entries (KeylessCache.py:27-38);
 *   0: no cache; < 0: empty the table (a new self-play round: the reference builds new Gamers, hence new caches).
 * stats out4: hits, misses, entries in use, table size. */
nz_status nz_scs_search_cache(nz_scs_search* h, int64_t max_entries);
nz_status nz_scs_search_cache_stats(nz_scs_search* h, int64_t* out4_host);
/* What the per-move records hold, bounded from the game description at create (the reference itself has no limits,
 * SCS_Game.py:395-484): decisions per game (= the M of nz_scs_search_export's [G, M] / [G, M, C] arrays) and children
 * per node (= C, a multiple of 64, at most 256; a description that allows more is rejected by nz_scs_search_create). */
nz_status nz_scs_search_limits(const nz_scs_search* h, int32_t* max_moves, int32_t* max_children);
/* simulation waves (kernel rounds) the last nz_scs_search_play took (persistent route: one launch per move) */
nz_status nz_scs_search_waves(const nz_scs_search* h, int64_t* waves);
/* The persistent route of nz_scs_search_play / _play_moves / _play_round: one wavefront per game runs the whole
 * search of a move -- descent, rules, the network for its own leaf, expansion, backup (Explorer.run_mcts,
 * Search/Explorer.py:40-67, with one simulation in flight per tree, :49-61) -- in ONE launch per move, no game waiting
 * for another.  Available, with or without the inference cache, for ConvNet / ResNet board nets
 *   - on boards of up to 32 cells, with layers of at most 64 channels and head layers no wider than the padded trunk,
 *   - whose input planes, padded to 16, fill whole 32-channel groups (17..32, 49..64, 81..96 or 113..128 planes: the
 *     86 of stacking limit 2, not the 67 and 105 of stacking limits 1 and 3),
 *   - one position of which fits a wavefront's 38 KB of LDS and four games' blocks a workgroup's 160 KB: with 86 planes
 *     up to 30 cells at widths of up to 32, up to 18 cells at widths 33..64 (DESIGN.md section 7 has the table);
 * other configurations keep the wave-by-wave route (the same games, slower).
 * enable: 1 require it (a play fails where it is not available), 0 never, -1 the default (use it where available).
 * *used (may be NULL): whether the last play ran on it. */
nz_status nz_scs_search_persistent(nz_scs_search* h, int32_t enable, int32_t* used);
/* Every game on its OWN map: the reference builds a new game object per game (Training/Gamer.py:52) and a "Randomized"
 * config draws terrain and victory points from numpy's global stream when that object is built (SCS_Game.py:1678-1738;
 * what most of the reference's SCS presets train on, Run.py:115).  Host arrays for n games (n >= the games of a round;
 * game i of a round reads row i whichever slot plays it): terrain float32 [n][tiles][3] (attack modifier, defense
 * modifier, cost), vp int32 [n][n_vp0 + n_vp1][2] (row, column), the counts as in the description passed to
 * nz_scs_search_create (its own map is then only a template: bound the limits with the cheapest terrain).  mt_keys
 * uint32 [n][624] + mt_pos int32 [n] (both or neither): the numpy RandomState state each game's stream goes on from --
 * where the map's draws left it, so that one stream serves map and search as in `np.random.seed(s); SCS_Game(cfg); play`;
 * the `seeds` of the play calls are then ignored (may be NULL).  n = 0: back to the description's one map.  Resets. */
nz_status nz_scs_search_set_games(nz_scs_search* h, int64_t n, const float* terrain_host, const int32_t* vp_host,
                                  const uint32_t* mt_keys_host, const int32_t* mt_pos_host);
/* The same per-game maps drawn by the library from seeds alone, on the device: what SCS_Game(config) draws for a
 * "Randomized" map or victory points (SCS_Game.py:1678-1738) after np.random.seed(seed), as the reference's Gamer does
 * per game (Training/Gamer.py:52).  nz_scs_search_set_map_draw sets, once per config, what a game draws:
 *   types [n_types][3]  attack modifier, defense modifier, cost of each terrain type in the Terrain section's order
 *                       (at most 32);
 *   cdf [n_types]       numpy's float64 p.cumsum() / p.cumsum()[-1] of the map's distribution (uniform when the config
 *                       gives none); a tile is types[searchsorted(cdf, random_sample(), 'right')] (legacy choice(p));
 *   order[2]            the randomized sections in the file's order: NZ_SCS_DRAW_MAP, NZ_SCS_DRAW_VP; 0 = none;
 *   number_vp[2]        points per side (as n_vp of the description), side_cols[4] the two sides' columns
 *                       [p1 first, p1 end, p2 first, p2 end) -- a point is (choice(range(rows)), choice(side's columns)),
 *                       redrawn while it repeats one of its side's.
 * Sections the config gives in "Detailed" form are the description's.  The caller validates the distribution (numpy's
 * ValueError); the library refuses a spec without randomized sections, counts unlike the description's, empty or bad
 * ranges and more points than a side has cells (keeping the spec set before).  NULL: no draw set.
 * nz_scs_search_draw_games: the effect of nz_scs_search_set_games with the maps and the streams RandomState(seeds[i])
 * gives -- bit for bit what the host draw gives, digests of the inference cache included.  seeds_host uint32 [n]
 * (n >= the games of a round); the per-game buffers are kept and grown across calls.  Returns when the maps are set
 * (the streams are built on the host from one copy of the MT19937 states).  Resets.
 * nz_scs_search_drawn_games: copies of the last draw (host or device pointers; any may be NULL): *n games, terrain
 * float32 [n][tiles][3], vp int32 [n][n_vp0 + n_vp1][2], the streams' state after the map: mt_keys uint32 [n][624],
 * mt_pos int32 [n] (numpy's RandomState.get_state() key and pos).  NZ_ERR_STATE when the games were not drawn here. */
#define NZ_SCS_DRAW_MAP 1
#define NZ_SCS_DRAW_VP 2
typedef struct nz_scs_map_draw {
  int32_t n_types;
  const float* types;
  const double* cdf;
  int32_t order[2];
  int32_t number_vp[2];
  int32_t side_cols[4];
} nz_scs_map_draw;
nz_status nz_scs_search_set_map_draw(nz_scs_search* h, const nz_scs_map_draw* spec);
nz_status nz_scs_search_draw_games(nz_scs_search* h, int64_t n, const uint32_t* seeds_host, void* stream);
nz_status nz_scs_search_drawn_games(nz_scs_search* h, int64_t* n, float* terrain, int32_t* vp, uint32_t* mt_keys,
                                    int32_t* mt_pos, void* stream);
/* As above for the rule operators: every game of the batch on its own map (NULL terrain: the description's).  Resets. */
nz_status nz_scs_set_maps(nz_scs* h, const float* terrain_host, const int32_t* vp_host, void* stream);
/* HIP-event timing of the persistent kernel, on the stream it is launched on.  enable: 1 on (sums zeroed), 0 off, -1 leave.
 * out4_host (may be NULL): milliseconds summed over launches, launches, v_mfma_f32_16x16x32_bf16 instructions issued
 * per evaluated position, algorithmic float32 FLOPs per position. */
nz_status nz_scs_search_persist_profile(nz_scs_search* h, int32_t enable, double* out4_host);
/* Test hook of the persistent route: keep the leaf evaluations of n games (games_host: indices), up to `capacity`
 * each, in the order the game's search consumed them; n = 0 stops.  nz_scs_search_record_read (host pointers, any of the
 * three arrays may be NULL): *count evaluations consumed, digests uint64 [.][2] (a 128-bit mix of the leaf's float32
 * planes), probs float32 [.][A] post-softmax, values float32 [.]; rows = min(*count, capacity). */
/* Diagnostic (library built with -DNZ_PERSIST_STAMPS; zeros otherwise): shader ticks of the persistent route summed over
 * games and moves since the last reset: clone, descent, legal mask + list, planes + split, network, softmax + value,
 * expansion, backup, whole moves, the slowest single (game, move); inside the network (leader's half): K loops,
 * epilogues, waits for the helper.  13 values. */
nz_status nz_scs_search_persist_ticks(nz_scs_search* h, int64_t* out13_host);
/* Diagnostic: the persistent route's network alone -- `blocks` workgroups of four (leader, helper) wavefront pairs each
 * run `iters` passes on an all-zero input; ticks_host[blocks * 4] = shader ticks per pass. */
nz_status nz_scs_netbench(nz_boardnet* net, int32_t blocks, int32_t iters, uint64_t* ticks_host);
/* Diagnostic (-DNZ_WIDE_STAMPS builds of the library only, NZ_ERR_STATE otherwise): phase ticks of conv_wide_kernel's K
 * steps summed over its launches so far -- [0] loads issued, [1] first fragments read, [2] MFMAs + staging, [3] barrier,
 * [4] loop overhead, [5] K steps, [6] launches, [7] 0.  No reference counterpart. */
nz_status nz_boardnet_wide_stamps(uint64_t* out8);
nz_status nz_scs_search_record(nz_scs_search* h, const int32_t* games_host, int32_t n, int32_t capacity);
nz_status nz_scs_search_record_read(nz_scs_search* h, int32_t slot, int32_t* count, uint64_t* digests_host,
                                    float* probs_host, float* values_host);

/* ---- evaluation matches between two MCTS agents on SCS, played inside the library -----------------------------------
 * Tester.Test_using_agents with two MctsAgents that keep their subtrees (Testing/Tester.py:46-121,
 * Testing/Agents/Generic/MctsAgent.py:28-39), n_games matches at once -- the trainer's "new network against the
 * previous checkpoint".  a1 / a2: two engines of ONE game description and the same number of games, both training = 0
 * and keep_subtree = 1, each with its own search config, its own network and its own trees; match g is game slot g of
 * both.  Agent 1 moves when the game's player index is 1 (as oracle/agents.py play_match restates Tester.py:62-118).
 * Per-game maps (nz_scs_search_set_games / _draw_games) must be set on BOTH handles and be the same maps: the rows' map
 * digests are compared and a difference is refused with NZ_ERR_ARG.
 * Per decision, for all live matches, on the device: both engines search the position (the mover's choose_action, the
 * opponent's update_subtree) -- each on the persistent route where its network has the per-wavefront form, wave by wave
 * otherwise, exactly as nz_scs_search_play decides (nz_scs_search_persistent, nz_scs_search_record and
 * nz_scs_search_cache work per handle as there; nz_scs_search_persist_profile is not summed here) -- agent 2's search on
 * a stream of its own between a fork and a join event; a hand-over kernel gives each engine's end_move its forced
 * actions (-1 for the match's mover, the mover's max_action for the opponent) and keeps the match record.  The host
 * waits once per decision, for the count of live matches and the engines' error flags.
 * The inference cache stays per handle: the two networks differ, so the two tables are never shared or merged.
 * max_moves > 0 stops every match after that many decisions (both engines at the same decision).  Synchronises.
 * Resets both engines; afterwards nz_scs_search_status / _export read either engine as after nz_scs_search_play.
 * nz_scs_match_result: the round's tally, counted on the device (terminal value +1: player 1 wins, -1: player 2 wins;
 * unfinished: stopped at max_moves; length_sum / length_max over all matches), and the match record actions_dev
 * int32 [n_games][M] (M of nz_scs_search_limits; -1 past the end; may be NULL).  Refuses (NZ_ERR_STATE) a round in which
 * the two engines' own records and the match record disagree anywhere. */
typedef struct nz_scs_match_tally {
  int64_t matches, p1_wins, p2_wins, draws, unfinished, length_sum, length_max;
} nz_scs_match_tally;
nz_status nz_scs_match_play(nz_scs_search* a1, nz_boardnet* net1, nz_scs_search* a2, nz_boardnet* net2,
                            int32_t max_moves, void* stream);
nz_status nz_scs_match_result(nz_scs_search* a1, nz_scs_search* a2, nz_scs_match_tally* out_host, int32_t* actions_dev,
                              void* stream);

/* ---- evaluation matches against scripted agents on SCS, played inside the library ----------------------------------
 * The cheaper tests a training run schedules (the bare policy against a random mover, MCTS against
 * a random mover, MCTS against the bare policy), n_games matches at once on ONE handle.  Agent p1 moves when the game's
 * player index is 1, p2 otherwise (as nz_scs_match_play).  The reference's Testing/Agents sources are not restated
 * anywhere in this repository: the two scripted agents follow harness rules (parity unpinned):
 *   NZ_AGENT_POLICY  at its own decisions evaluates the current position with `net` (its recurrent iterations as set)
 *                    and plays the legal action with the largest softmax probability, the lowest flat action index
 *                    winning a tie (np.argmax); no search, no tree, nothing on the opponent's turn;
 *   NZ_AGENT_RANDOM  match i owns the stream np.random.RandomState(seeds_host[i]) (uint32 [n_games]; apart from the
 *                    map's stream); at its own decision with n legal actions it draws k = rs.randint(n) (the legacy
 *                    masked rejection on 32-bit words; n == 1 draws nothing) and plays the k-th legal action in
 *                    ascending flat action index; nothing is drawn on the opponent's turn;
 *   NZ_AGENT_MCTS    `h`'s own search with `net` (training = 0, keep_subtree = 1; the persistent route where available,
 *                    exactly as nz_scs_search_play decides; nz_scs_search_persistent / _record / _cache work as there):
 *                    it searches on every ply (its own choose_action, the opponent's update_subtree) and follows the
 *                    scripted mover's action through nz_scs_search_apply's forced actions.
 * At most one side is NZ_AGENT_MCTS; two are refused with NZ_ERR_ARG (each MCTS agent needs its own trees:
 * nz_scs_match_play).  Without an MCTS side no simulation runs at all: the agents' kernel steps the games and keeps
 * the handle's action record, and the trees stay the unexpanded roots of the reset.  Per decision, for all live
 * matches, on the device: the MCTS side's search; each policy agent's positions written into its network's input rows
 * and evaluated on a device-side count, one side after the other on `stream`, so the two sides may share one network
 * object in any pairing (policy against policy included); one wavefront per match decides for the scripted mover.  The
 * host waits once per decision, for the count of live matches, the engine's error flag and the agents' error words
 * (a randint rejection cap or a live position without a legal action is NZ_ERR_OVERFLOW).  Per-game maps: as set on
 * `h`.
 * max_moves > 0 stops every match after that many decisions.  Resets `h`; the random agents' streams are rebuilt from
 * the seeds, so a round is a function of its arguments.  Synchronises.  Afterwards nz_scs_search_status / _export read
 * `h` as after nz_scs_search_play (a handle without an MCTS side holds the actions only, and 0 simulations).
 * nz_scs_agent_match_result: the tally and the match record as nz_scs_match_result gives them.
 * nz_scs_agent_match_decisions: a scripted side's (0: p1, 1: p2) decisions by the game's decision number, device
 * pointers [n_games][M] (M of nz_scs_search_limits), any may be NULL: actions (-1 where the side did not decide), the
 * legal actions it chose from, and for the policy agent the winning probability.
 * nz_scs_agent_record / _record_read: the test hook of nz_scs_search_record / _record_read for a policy side -- the
 * (digest, probs, value) rows of the chosen matches in the order the agent consumed them. */
enum { NZ_AGENT_MCTS = 0, NZ_AGENT_POLICY = 1, NZ_AGENT_RANDOM = 2 };
typedef struct nz_scs_agent {
  int32_t kind;
  nz_boardnet* net;            /* policy and MCTS agents */
  const uint32_t* seeds_host;  /* random agents: [n_games] */
} nz_scs_agent;
nz_status nz_scs_agent_match_play(nz_scs_search* h, const nz_scs_agent* p1, const nz_scs_agent* p2, int32_t max_moves,
                                  void* stream);
nz_status nz_scs_agent_match_result(nz_scs_search* h, nz_scs_match_tally* out_host, int32_t* actions_dev, void* stream);
nz_status nz_scs_agent_match_decisions(nz_scs_search* h, int32_t side, int32_t* actions_dev, int32_t* n_legal_dev,
                                       float* probs_dev, void* stream);
nz_status nz_scs_agent_record(nz_scs_search* h, int32_t side, const int32_t* games_host, int32_t n, int32_t capacity);
nz_status nz_scs_agent_record_read(nz_scs_search* h, int32_t side, int32_t slot, int32_t* count, uint64_t* digests_host,
                                   float* probs_host, float* values_host);

/* ---- SCS evaluation matches from opening positions ---------------------------------------------------------------------
 * Evaluation agents are deterministic (no noise, max action), so on ONE map nz_scs_match_play with two MCTS agents, or
 * nz_scs_agent_match_play with MCTS against the bare policy, plays one game n_games times.  The remedy that leaves the
 * game alone: start match g at the position a prefix of g's own actions leads to.  No reference counterpart (harness
 * rules); Tic-Tac-Toe's twin is nz_engine_match_play_from.
 * nz_scs_openings (host memory, copied before the call returns): actions int32 [n_games][max_plies], match g's prefix
 * in its first n_plies[g] entries (the rest is not read); n_plies int32 [n_games], NULL: every match has max_plies.
 * nz_scs_search_reset_to: nz_scs_search_reset, then one wavefront per match replays the prefix through the legal mask
 * and the step.  Afterwards match g stands at its position, its tree is the unexpanded root (MctsAgent.new_game, then
 * choose_action, on a game stepped there), and its records hold the prefix at the game's own decision numbers:
 * actions [g][ply] of nz_scs_search_export, n_children and tree_size 0 for those plies (nobody searched them);
 * nz_scs_search_last_actions gives the prefix's last action.  NULL openings or max_plies == 0 is nz_scs_search_reset
 * itself.  Refused with NZ_ERR_ARG before any launch, the engine untouched: a NULL handle or actions, max_plies < 0 or
 * above max_moves of nz_scs_search_limits, an n_plies[g] outside 0 .. max_plies, an action outside 0 .. A-1 within a
 * match's plies (the message names match and ply).  The call then synchronises and reads one error word per match: an
 * action that is not legal in its position, or a game that ended before its prefix did, returns NZ_ERR_ARG with the
 * first such match, its ply, action and reason in nz_scs_search_last_error, and the engine is left as after
 * nz_scs_search_reset: nothing of a refused call survives.
 * nz_scs_match_play_from / nz_scs_agent_match_play_from: nz_scs_match_play / nz_scs_agent_match_play with every match
 * started at its opening, the same openings in both engines of a match; the functions without _from are their NULL
 * case and enqueue exactly what they always did.  Refused openings are refused before anything is reset.  max_moves
 * counts the round's own decisions, not the opening's plies.  The mover rule is unchanged (agent 1 moves for player
 * index 1), so a prefix decides who moves first.  A random side's stream starts fresh at its first own decision after
 * the opening.  The match record, the engines' records and nz_scs_agent_match_decisions stay indexed by the game's
 * decision number; the match record holds the opening's plies there (a scripted side's own record holds -1 / 0: it did
 * not decide them), so the tally's check for gaps stands as it is.
 * nz_scs_openings_draw: match g owns np.random.RandomState(seeds_host[g]) (uint32 [n_games]; a stream apart from the
 * map's and the random agents') and plays the random agent's rule from the start -- k = rs.randint(n_legal), n_legal ==
 * 1 draws nothing, the k-th legal action in ascending flat index -- for `plies` plies (1 .. max_moves) or to the
 * game's end, on the match's own map where maps are per game.  Host outputs: actions_out int32 [n_games][plies] (-1 past
 * a prefix's end), n_plies_out int32 [n_games].  Touches no game of the engine.  Synchronises.
 * nz_scs_openings_expand: one level of the enumeration of all openings.  frontier_host int32 [n_prefixes][depth]
 * (depth >= 0; depth 0: the start, frontier_host may be NULL): each prefix is replayed from the start.  counts_host
 * int32 [n_prefixes] receives the number of legal actions after each prefix (0: the game is over there, or it is a live
 * position without a legal action -- a placement whose every arrival tile the enemy holds).  With
 * children_host non-NULL (keys_host too) the call also writes, at the exclusive scan of the counts, the child prefixes
 * children_host int32 [sum of counts][depth + 1] in ascending action order and keys_host uint64 [sum of counts][2],
 * the 128-bit digest of each child position's planes (the digest nz_scs_search_record_read reports for a leaf; equal
 * keys: positions the network and the rules cannot tell apart, so the two orders of placing two units of one type count
 * once -- the inference cache's state hash would tell them apart) -- call once without them to size the arrays.  A prefix that is not a
 * legal sequence is NZ_ERR_ARG naming prefix and ply.  Refused with NZ_ERR_STATE while per-game maps are set: one
 * frontier belongs to one map.  Touches no game of the engine.  Synchronises. */
typedef struct nz_scs_openings {
  const int32_t* actions;
  const int32_t* n_plies;
  int32_t max_plies;
} nz_scs_openings;
nz_status nz_scs_search_reset_to(nz_scs_search* h, const nz_scs_openings* openings, void* stream);
nz_status nz_scs_match_play_from(nz_scs_search* a1, nz_boardnet* net1, nz_scs_search* a2, nz_boardnet* net2,
                                 const nz_scs_openings* openings, int32_t max_moves, void* stream);
nz_status nz_scs_agent_match_play_from(nz_scs_search* h, const nz_scs_agent* p1, const nz_scs_agent* p2,
                                       const nz_scs_openings* openings, int32_t max_moves, void* stream);
nz_status nz_scs_openings_draw(nz_scs_search* h, const uint32_t* seeds_host, int32_t plies, int32_t* actions_out,
                               int32_t* n_plies_out, void* stream);
nz_status nz_scs_openings_expand(nz_scs_search* h, const int32_t* frontier_host, int32_t n_prefixes, int32_t depth,
                                 int32_t* counts_host, int32_t* children_host, uint64_t* keys_host, void* stream);

/* ---- Tic-Tac-Toe evaluation matches played inside the library ---------------------------------------------------------
 * Tester.Test_using_agents on Tic-Tac-Toe: n_games matches between side 1 (moves for player 1, the first mover, as in
 * oracle/agents.py play_match) and side 2, each an NZ_AGENT_MCTS, NZ_AGENT_POLICY or NZ_AGENT_RANDOM.  The scripted
 * agents follow the harness rules of nz_scs_agent_match_play (parity unpinned):
 *   NZ_AGENT_MCTS    an engine created with training = 0 (keep_subtree = 1) with weights or a table: it searches on every
 *                    ply (its own choose_action, the opponent's update_subtree) and follows the other side's action as
 *                    nz_engine_apply(actions_dev) takes it;
 *   NZ_AGENT_POLICY  an engine (training = 0) of which only the network or table is used: at its own plies the current
 *                    position is evaluated and the legal cell of largest softmax probability is played, the lowest cell
 *                    index winning a tie (np.argmax).  Two policy sides may share one engine;
 *   NZ_AGENT_RANDOM  engine NULL; match i owns np.random.RandomState(agent_seeds[i]) (uint32 [n_games]), draws
 *                    k = rs.randint(n_legal) at its own plies (n_legal == 1 draws nothing) and plays the k-th empty cell
 *                    in ascending index.
 * At least one side has an engine (it gives the number of matches).  Refused with NZ_ERR_ARG (message in nz_last_error of
 * every engine passed, and of NULL) before any launch: a missing engine or one passed for a random side, one engine on
 * both sides unless both are policy sides, engines with different game counts or devices or with n_slots != n_games, a
 * training engine, missing seeds for a random side, an MCTS or policy side without weights or table.
 * The call resets the engines, enqueues exactly nine plies on `stream` -- per ply the search of every MCTS side, for a
 * scripted mover its evaluation and the agents' kernel, then the apply of every MCTS side; finished matches are no-ops --
 * then the tally, and synchronises `stream` once at the end: no host read-back between plies.
 * `out` (may be NULL; every pointer in it may be NULL) receives, in DEVICE memory: actions int32 [n][9] (-1 past the
 * end), lengths [n], outcomes [n] (the terminal value: +1 player 1 won, -1 player 2 won, 0 draw), per side
 * agent_actions / agent_n_legal int32 [n][9] by ply (-1 / 0 where that side did not decide or is an MCTS side); and in
 * HOST memory tally4_host int64 [4]: side-1 wins, side-2 wins, draws, unfinished.
 * nz_engine_match_streams (test hook): the MT19937 state (key uint32 [n][624], pos int32 [n], host memory) in which the
 * last match round left random side `side` (0 / 1); `e` is that round's first non-NULL engine. */
typedef struct nz_ttt_match_result {
  int32_t* actions;
  int32_t* lengths;
  int32_t* outcomes;
  int32_t* agent_actions[2];
  int32_t* agent_n_legal[2];
  int64_t* tally4_host;
} nz_ttt_match_result;
nz_status nz_engine_match_play(nz_engine* side1, int32_t kind1, nz_engine* side2, int32_t kind2,
                               const uint32_t* agent_seeds1_host, const uint32_t* agent_seeds2_host,
                               const nz_ttt_match_result* out, void* stream);
nz_status nz_engine_match_streams(nz_engine* e, int32_t side, uint32_t* keys_host, int32_t* pos_host);

/* nz_engine_match_play from given positions: match i starts at start_boards_host[i] (uint32 [n_games], host memory;
 * the playable positions of nz_engine_reset_to), every MCTS side from a fresh root there.  NULL is nz_engine_match_play,
 * which is this call.  All of nz_engine_match_play's refusals stand and come first; then NZ_ERR_ARG for a board that
 * is not playable (index and condition named) and for start boards that do not all hold the same number of stones k
 * (both counts named): every match of a round is at the same ply, which is what lets the host enqueue the round
 * without a read-back.  Plies k .. 8 are enqueued; side 1 still moves for player 1, the even plies, so with odd k
 * side 2 moves first.  The match's record stays by absolute ply: actions[i][p] is -1 for p < k and past the end,
 * lengths[i] the stone count of the final position, agent_actions / agent_n_legal by ply as before.  An MCTS side's
 * engine counts from the position (nz_engine_reset_to): its record is the match's shifted by k.
 * nz_engine_policy_actions: the bare-policy agent's decision on each of n <= n_games playable positions (boards_host
 * uint32 [n], host memory) into actions_dev (int32 [n], device memory; enqueued on `stream`, no synchronisation): the
 * legal cell of largest softmax probability from the engine's network or table, the lowest index on a tie -- the
 * policy mover of the matches, run on the engine's match state (a later nz_engine_match_streams is refused).  Refused
 * with NZ_ERR_ARG: a NULL argument, n outside 1 .. n_games, no network or table, a board that is not playable. */
nz_status nz_engine_match_play_from(nz_engine* side1, int32_t kind1, nz_engine* side2, int32_t kind2,
                                    const uint32_t* agent_seeds1_host, const uint32_t* agent_seeds2_host,
                                    const uint32_t* start_boards_host, const nz_ttt_match_result* out, void* stream);
nz_status nz_engine_policy_actions(nz_engine* e, const uint32_t* boards_host, int32_t n, int32_t* actions_dev,
                                   void* stream);

/* ---- host random streams (numpy legacy RandomState, MT19937) --------------
 * Replaces the reference's use of the global np.random stream
 * (Explorer.py:77-78,89,199,208). */
nz_rng* nz_rng_create(uint32_t seed);
/* a stream that goes on where a numpy RandomState stands (RandomState.get_state(): key[624], pos, has_gauss, cached_gaussian) */
nz_rng* nz_rng_create_state(const uint32_t* key624, int32_t pos, int32_t has_gauss, double cached_gaussian);
nz_rng* nz_rng_clone(const nz_rng* r);
void nz_rng_destroy(nz_rng* r);
void nz_rng_seed(nz_rng* r, uint32_t seed);
uint32_t nz_rng_u32(nz_rng* r);
double nz_rng_double(nz_rng* r);                                  /* random_sample() */
void nz_rng_gamma(nz_rng* r, double shape, double scale, int32_t n, double* out);  /* gamma(shape, scale, n) */

/* ---- replay buffer on the device ------------------------------------------
 * The positions of finished games stay in HBM; which physical slot a position takes and which slots a batch reads
 * is decided by the caller (host logic of Training/ReplayBuffer.py:24-53: window in games with per-position
 * eviction, shuffle, slice, sample), the library moves the data:
 *   nz_replay_append  replaces the tuple building of ReplayBuffer.save_game (ReplayBuffer.py:31-36) together with
 *                     Game.store_search_statistics / make_target (tic_tac_toe.py:177-190, SCS_Game.py:1517-1528):
 *                     row r of the source (state + the root's visit counts, or ready-made policies, or per-child
 *                     (action, visit) lists) becomes the position in slot dst_slot[r] (-1: not stored); policy =
 *                     visit / sum(visits) in double, rounded to float32 as torch.tensor() does (AlphaZero.py:901);
 *                     value = game_value[r / rows_per_game].
 *   nz_replay_gather  replaces batch assembly (AlphaZero.py:846-852,892-903: torch.cat of the states, one
 *                     torch.tensor per target): states [B, state_floats], policies [B, A], values [B], game_index [B]
 *                     for the physical slots of a batch, in the order given (the caller groups by game index).
 * All pointers are device pointers; work is enqueued on `stream`. */
typedef struct nz_replay nz_replay;
nz_status nz_replay_create(nz_replay** out, int64_t capacity_positions, int32_t state_floats, int32_t num_actions,
                           int32_t device);
void nz_replay_destroy(nz_replay* h);
const char* nz_replay_last_error(const nz_replay* h);
nz_status nz_replay_dims(const nz_replay* h, int64_t* capacity, int32_t* state_floats, int32_t* num_actions);
/* nz_replay_create: NZ_ERR_ARG for a NULL `out` or a size <= 0, NZ_ERR_HIP where `device` is no HIP device or the
 * allocation fails (*out stays NULL; the message is read with nz_replay_last_error(NULL)).
 *
 * nz_replay_append: exactly one of visits_dev [N, A] int32 / policies_dev [N, A] float32 / (child_action_dev,
 * child_visit_dev [N, max_children] int32 + n_children_dev [N]); game_value_dev holds one int32 per rows_per_game rows
 * (the last game may have fewer).  NZ_ERR_ARG, with a message and nothing enqueued, for a NULL handle, states, values or
 * slots, for none or more than one of the three forms, for child lists without visits, counts or max_children > 0, and for
 * rows_per_game <= 0; n_rows <= 0 (and batch <= 0 in nz_replay_gather) is NZ_OK and does nothing.  Per row:
 *   dst_slot = -1 (any negative slot) leaves the buffer alone;
 *   dst_slot >= capacity raises flag 1, the row is not stored;
 *   dense and sparse form: an action with 0 visits gets policy 0, also where the row's visits sum to 0 (never 0 / 0);
 *   sparse form: only the first n_children[r] entries of row r's lists are read.  A child whose action is outside
 *   0 .. A-1 raises flag 2 and is skipped (its visits still count in the row's sum); a count n_children[r] outside
 *   0 .. max_children raises flag 2 and counts as 0 -- the row's state, value and game index are still stored, its policy
 *   is zeros.  The rows of one call must name distinct slots, a row's children distinct actions.
 * nz_replay_gather: each of the four outputs may be NULL; a slot outside 0 .. capacity-1 raises flag 4 and leaves that
 * row of the outputs as it was; slots may repeat.
 * The flags are one device word, OR-ed by the kernels.  nz_replay_check synchronises `stream` and returns
 * NZ_ERR_OVERFLOW, with the word in the message, while any flag is set: 1 slot at or beyond capacity, 2 action or child
 * count out of range, 4 batch slot out of range.  The word is sticky: checking does not clear it, a handle that has raised
 * a flag reports it from every later check until it is destroyed. */
nz_status nz_replay_append(nz_replay* h, const float* states_dev, const int32_t* visits_dev, const float* policies_dev,
                           const int32_t* child_action_dev, const int32_t* child_visit_dev, const int32_t* n_children_dev,
                           int32_t max_children, const int32_t* game_value_dev, int32_t rows_per_game,
                           const int64_t* dst_slot_dev, int64_t n_rows, int32_t game_index, void* stream);
nz_status nz_replay_gather(nz_replay* h, const int64_t* slots_dev, int64_t batch, float* states_out, float* policies_out,
                           float* values_out, int32_t* game_index_out, void* stream);
/* synchronises; NZ_ERR_OVERFLOW if a kernel has seen a slot, an action or a child count out of range (sticky, see above) */
nz_status nz_replay_check(nz_replay* h, void* stream);

/* ---- compact SCS replay buffer ("states as compact game state re-rendered") ----------
 * A second buffer beside nz_replay for SCS games: a slot holds the game STATE the position was, not its image, and the
 * gather renders the image.  A record is self-contained:
 *   int32 n_children, float value, int32 game_index | float terrain[tiles][3] (the game's own map, the image's values) |
 *   {int32 action, float policy}[max_children] (the root's child list) | the rules' state struct (640 bytes) |
 *   int8 victory-point tiles [2 * tiles reserved]
 * 1.5 KB on a 5x5 board with 64 children, 4.1 KB on 10x10 with 256, against 10.7 KB and 42.8 KB of a dense row.  Slots
 * are assigned by the caller exactly as for nz_replay.  All array arguments are device pointers unless named _host;
 * work is enqueued on `stream`. */
typedef struct nz_scs_replay nz_scs_replay;
/* Host code, no device needed: the bytes of one record for boards of `desc`'s shape with `max_children` child entries
 * (<= 0: the description's own bound on the legal actions of a position, rounded up to a multiple of 64 as the search
 * engine's records round it).  -1, with a message for the last-error call with NULL, for a description the rules refuse
 * or a max_children below the description's bound. */
int64_t nz_scs_replay_record_bytes(const nz_scs_desc* desc, int32_t max_children);
/* `capacity_positions` records of `max_children` child entries for images [channels][rows][cols] and `num_actions`
 * actions (they must be an SCS shape: channels = 48 + 19 * stacking, actions = (3 + 9 * stacking) * rows * cols).
 * NZ_ERR_ARG for sizes that are none, NZ_ERR_HIP where `device` is no HIP device or the allocation fails. */
nz_status nz_scs_replay_create(nz_scs_replay** out, int64_t capacity_positions, int32_t max_children, int32_t channels,
                               int32_t rows, int32_t cols, int32_t num_actions, int32_t device);
void nz_scs_replay_destroy(nz_scs_replay* h);
const char* nz_scs_replay_last_error(const nz_scs_replay* h);
nz_status nz_scs_replay_dims(const nz_scs_replay* h, int64_t* capacity, int32_t* record_bytes, int32_t* max_children,
                             int32_t* num_actions);
/* The game description of `game_index` (0 .. 15), which is what the trainer buckets batches by.  NZ_ERR_ARG: rows,
 * columns, action planes or channels differ from the buffer's; the description's bound on a position's legal actions
 * exceeds the buffer's max_children; the index already has a DIFFERENT description (the same one again is NZ_OK). */
nz_status nz_scs_replay_register(nz_scs_replay* h, int32_t game_index, const nz_scs_desc* desc);
/* Replays the first `n_games` games of a finished round from their recorded actions [G][max_moves] (lengths [G],
 * outcomes [G] int32; terrain float [G][tiles][3] and vp int32 [G][n_vp0 + n_vp1][2] for per-game maps, or both NULL),
 * one wavefront per game, and stores nothing.  Before every step the action must be inside 0 .. A-1 and legal; a game
 * that reached its end must have the recorded outcome; a game that stops before its end is accepted as it is.
 * Synchronises; NZ_ERR_ARG with "game G, move M: ..." for the first record that fails. */
nz_status nz_scs_replay_check_games(nz_scs_replay* h, int32_t game_index, int64_t n_games, const int32_t* actions_dev,
                                    int32_t max_moves, const int32_t* lengths_dev, const int32_t* outcomes_dev,
                                    const float* terrain_dev, const int32_t* vp_dev, void* stream);
/* The same replay in one launch, storing move m of game g in slot dst_slot_dev[g][m] (int64 [G][dst_stride]; negative,
 * or m >= dst_stride: not stored).  Child lists as the search engine exports them: child_action / child_visit int32
 * [G][max_moves][round_children], n_children [G][max_moves]; policy = (float)((double)visit / (double)sum of visits),
 * 0 for a zero visit count, as the dense buffer's append forms it.  Meant to follow a clean check of the same round: a
 * record the check would refuse stops its game's replay and raises flag 8. */
nz_status nz_scs_replay_save(nz_scs_replay* h, int32_t game_index, int64_t n_games, const int32_t* actions_dev,
                             int32_t max_moves, const int32_t* lengths_dev, const int32_t* outcomes_dev,
                             const float* terrain_dev, const int32_t* vp_dev, const int32_t* child_action_dev,
                             const int32_t* child_visit_dev, const int32_t* n_children_dev, int32_t round_children,
                             const int64_t* dst_slot_dev, int32_t dst_stride, void* stream);
/* states [B][channels][rows][cols], policies [B][A], values [B], game indices [B] of the slots of a batch, one wavefront
 * per row; each output may be NULL.  A slot outside 0 .. capacity-1 raises flag 4 and leaves its row as it was. */
nz_status nz_scs_replay_gather(nz_scs_replay* h, const int64_t* slots_dev, int64_t batch, float* states_out,
                               float* policies_out, float* values_out, int32_t* game_index_out, void* stream);
/* synchronises; NZ_ERR_OVERFLOW while the sticky error word is set: 1 slot at or beyond capacity, 2 child count or child
 * action out of range, 4 batch slot out of range, 8 unchecked record in a save, 16 a slot's game index has no description,
 * 32 a slot's state or map points outside the board (never saved, or a damaged checkpoint; the row is left as it was) */
nz_status nz_scs_replay_check(nz_scs_replay* h, void* stream);
/* the raw records of slots 0 .. n-1 to / from a device byte buffer of n * record_bytes (checkpoints) */
nz_status nz_scs_replay_export_slots(nz_scs_replay* h, int64_t n, void* bytes_dev, void* stream);
nz_status nz_scs_replay_import_slots(nz_scs_replay* h, int64_t n, const void* bytes_dev, void* stream);

/* ---- batched loss ---------------------------------------------------------------
 * AlphaZero.calculate_loss (Training/AlphaZero.py:891-921) for a whole batch in one launch, with the gradients of the
 * combined loss: losses3 = (value_loss, policy_loss, combined_loss); dlogits [B, A], dvalues [B] may be NULL.
 * policy_loss: cross entropy with label smoothing 0.02 (AlphaZero.py:327), KL divergence, masked MSE
 * (Utils/Functions/loss_functions.py:7-26); value_loss: squared / absolute error (loss_functions.py:28-33);
 * normalize_policy: divide the policy loss by log(batch) as the reference does (AlphaZero.py:912-915).
 * workspace_dev: 2 * batch floats.  Sums in a fixed order: the same inputs give the same bits.  float32 per element, the
 * sums behind the three losses carried in double (a small KL divergence is the difference of two sums of size log A);
 * log_softmax as (x - max) - log(sum exp(x - max)), so a common offset of the logits costs nothing.  Held to the
 * reference's loop in float64 (tests/test_gpu_loss_edges.py: 1 <= A <= 2100, batches up to 2048, logits 2 N, 30 N,
 * 2 N + 1e4, all equal, one entry +80; sparse, one-hot and dense targets): the losses within 2e-6 relative, which is
 * where the reference's own float32 loop sits; the gradients within 2e-6 of their largest entry, EXCEPT where float32
 * softmax itself has no more to give -- rows saturated by |logits| of 30 and more, whose whole gradient is ~1e-10 of
 * 1 / batch (there: within 2e-6 / batch absolute, or 4 x the error of the reference's float32 loop on the same row).  These are
 * the bounds the test asserts; DESIGN.md section 2 statement 12 says what has been measured on a device.
 * Masked MSE with a target row of zeros only (the reference raises ZeroDivisionError there): losses3[1] and [2] come out
 * NaN, that sample's dlogits row is zeros. */
enum { NZ_LOSS_CE = 0, NZ_LOSS_KLD = 1, NZ_LOSS_MSE = 2 };
enum { NZ_LOSS_SE = 0, NZ_LOSS_AE = 1 };
nz_status nz_loss_forward_backward(const float* logits_dev, const float* values_dev, const float* target_policies_dev,
                                   const float* target_values_dev, int32_t batch, int32_t actions, int32_t policy_loss,
                                   int32_t value_loss, int32_t normalize_policy, float* losses3_dev, float* dlogits_dev,
                                   float* dvalues_dev, float* workspace_dev, void* stream);
const char* nz_loss_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* NUZERO_AMD_H */
