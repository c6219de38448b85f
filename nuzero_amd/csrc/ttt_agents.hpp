// Tic-Tac-Toe evaluation matches (nz_engine_match_play, engine.hip): the match's own state and what the host hands to
// the kernels of ttt_agents.hip.  A match's position lives here, apart from the MCTS engines' games, which follow it
// move by move through nz_engine_apply's forced actions; a policy or random side has no game of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nz {

// per-match error word: the randint rejection cap was reached; a live position without an empty cell; the mover's
// action is not an empty cell (an MCTS side's record out of step with the match)
enum : int32_t { TTT_AGENT_ERR_CAP = 1, TTT_AGENT_ERR_NO_LEGAL = 2, TTT_AGENT_ERR_ACTION = 4 };

struct TttMatchArgs {
  int32_t n;                     // matches
  uint32_t* board;               // [n] player-one stones | player-two stones << 16 (tree_dev.hpp)
  int32_t* alive;                // [n]
  int32_t* length;               // [n]
  int32_t* outcome;              // [n] terminal value: +1 player 1, -1 player 2, 0 draw (and while unfinished)
  int32_t* actions;              // [n][9], -1 past the end
  int32_t* forced;               // [n] this ply's action: what every engine's apply takes (ignored for a finished match)
  int32_t* err;                  // [n] TTT_AGENT_ERR_*
  int32_t* agent_actions[2];     // [n][9] by ply; -1 where the side did not decide
  int32_t* agent_n_legal[2];     // [n][9] by ply; 0 where the side did not decide
  uint32_t* mt_keys[2];          // [n][624] random side's streams
  int32_t* mt_pos[2];            // [n]
  float* states;                 // [n][2][9] the policy mover's network input
  const float* probs;            // [n][9] its post-softmax output
};

// start: [n] the matches' start positions (playable, checked by the host; lengths begin at their stone counts), or
// nullptr for the empty board
void ttt_match_reset_launch(const TttMatchArgs& a, const uint32_t* start, hipStream_t s);
// the policy mover's network input: every live match's position as two planes (finished matches: zeros)
void ttt_state_image_launch(const TttMatchArgs& a, hipStream_t s);
// the scripted mover's decision for every live match: side 0 / 1, kind NZ_AGENT_POLICY (probabilities from `table`'s row
// of the position when there is one, else from a.probs) or NZ_AGENT_RANDOM
void ttt_agent_move_launch(const TttMatchArgs& a, int side, int kind, const float* table, hipStream_t s);
// every live match takes a.forced (from the agents' kernel or the MCTS mover's last action): record, step, end
void ttt_match_step_launch(const TttMatchArgs& a, hipStream_t s);
// tally [8] (zeroed by the host): side-1 wins, side-2 wins, draws, unfinished, the OR of the matches' error words, and
// the two engines' error flags (nullptr: none)
void ttt_match_tally_launch(const TttMatchArgs& a, const int32_t* flag1, const int32_t* flag2, unsigned long long* tally,
                            hipStream_t s);

}  // namespace nz
