// The scripted evaluation agents of nz_scs_agent_match_play (scs_agents.hip): what the match loop in scs_search.hip
// hands to their kernels.  One wavefront per live match acts for the side that is not an MCTS agent.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scs_dev.hpp"
#include "scs_mt.hpp"

namespace nz {

// per-match error word: the randint rejection cap was reached; a live position without a legal action; a game longer
// than the records' bound
enum : int32_t { AGENT_ERR_CAP = 1, AGENT_ERR_NO_LEGAL = 2, AGENT_ERR_LENGTH = 4 };

struct AgentSide {
  int32_t kind;                  // NZ_AGENT_*
  // policy agent: its network's input rows (nz_boardnet_input_rows), the evaluations by slot, the positions queued this decision
  float* net_rows;
  int32_t row_stride;
  const float* probs;            // [G][A] post-softmax
  const float* value;            // [G]
  int32_t* count;                // [1]
  // random agent: each match's MT19937 state between its decisions
  uint32_t* mt_keys;             // [G][624]
  int32_t* mt_pos;               // [G]
  // the side's decisions [G][max_moves], by the game's decision number (-1 / 0 where the side did not decide)
  int32_t* rec_action;
  int32_t* rec_n_legal;
  float* rec_prob;               // the winning probability (policy agent)
  // test hook (nz_scs_agent_record): the policy agent's evaluations of chosen matches in the order consumed
  const int32_t* hook_slot;      // [G] slot or -1; nullptr: off
  int32_t hook_cap;
  int32_t* hook_count;           // [slots]
  uint64_t* hook_digest;         // [slots][cap][2]
  float* hook_probs;             // [slots][cap][A]
  float* hook_value;             // [slots][cap]
};

struct AgentArgs {
  const ScsRules* rules;         // as SearchParams: one row, or one per match (rules_row)
  const int32_t* rules_row;
  ScsState* real;                // [G] the search handle's games
  int32_t n_games, max_moves, num_actions;
  int32_t step;                  // no MCTS side: the agents' kernel steps the games itself and keeps the handle's action record
  AgentSide side[2];             // [0] moves when the game's player index is 1 (oracle/agents.py play_match), [1] otherwise
  int32_t* forced;               // [G] what nz_scs_search_apply's kernel takes: the scripted mover's action, -1 where the MCTS side moves
  int32_t* rec_action;           // [G][max_moves] the handle's action record (written here only with `step`)
  int32_t* slot;                 // [G] evaluation slot of the match's position this decision
  uint64_t* digest;              // [G][2] digest of that position's planes (hooked matches)
  int32_t* err;                  // [G] AGENT_ERR_*
};

// (streams of the random agents: scs_mt.hpp's agent_seed_launch)
// out3 (zeroed by the host): live matches, the handle's error flag, the OR of the matches' error words
hipError_t agent_live_launch(const ScsState* real, int n, const int32_t* error_flag, const int32_t* err, int32_t* out3,
                             hipStream_t stream);
// the positions policy side `side` (0 / 1) decides this decision, as input rows of its network (count zeroed by the host)
hipError_t agent_image_launch(const AgentArgs& a, int side, hipStream_t stream);
// the scripted movers' decisions: forced actions, records, and with a.step the games' step
hipError_t agent_act_launch(const AgentArgs& a, hipStream_t stream);

}  // namespace nz
