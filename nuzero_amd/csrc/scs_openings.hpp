// Evaluation matches from opening positions (scs_openings.hip): what nz_scs_search_reset_to, nz_scs_openings_draw and
// nz_scs_openings_expand in scs_search.hip hand to the opening kernels.  One wavefront per match or prefix; the rules
// row and the game are in LDS, the legal mask, the step and the random stream are scs_dev.hpp's and scs_mt.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scs_dev.hpp"

namespace nz {

// A per-match (per-prefix) error word: 0, or (ply << 8) | reason -- the first violation, at which the wavefront stopped.
enum : int32_t {
  OPENING_ERR_ILLEGAL = 1,     // the action is not a legal action of the position (or not an action at all)
  OPENING_ERR_GAME_OVER = 2,   // the game ended before the prefix did
  OPENING_ERR_LENGTH = 3,      // the prefix runs past the decisions the records hold
  OPENING_ERR_NO_LEGAL = 4,    // draw: a live position without a legal action
  OPENING_ERR_CAP = 5,         // draw: the randint rejection cap
};
inline int opening_err_ply(int32_t e) { return (int)((uint32_t)e >> 8); }
inline int opening_err_reason(int32_t e) { return e & 0xff; }

struct OpeningGames {            // whose rules the prefixes are replayed under
  const ScsRules* rules;         // as SearchParams: one row, or one per match (rules_row)
  const int32_t* rules_row;      // [n] or nullptr: all read row 0
  int32_t num_actions;
};

// Apply: match g < n replays actions[g][0 .. n_plies[g]) (stride max_plies) from real[g], which the slot's reset has
// just set to the start.  A sound prefix leaves real[g] at its position and rec_action[g][ply] (stride max_moves) at its
// actions; a bad one leaves both alone and sets err[g].  err [n] is written for every match.
hipError_t opening_apply_launch(const OpeningGames& og, int n, const int32_t* actions, const int32_t* n_plies, int max_plies,
                                ScsState* real, int32_t* rec_action, int max_moves, int32_t* err, hipStream_t stream);

// Draw: match g < n owns RandomState(seeds[g]) and plays the random agent's rule from the start for `plies` plies or to
// the game's end: actions_out [n][plies] (-1 past the prefix's end), n_plies_out [n], err [n].  No engine state is touched.
hipError_t opening_draw_launch(const OpeningGames& og, int n, const uint32_t* seeds, int plies, int32_t* actions_out,
                               int32_t* n_plies_out, int32_t* err, hipStream_t stream);

// Expand: prefix f < n of `depth` plies (frontier [n][depth]) is replayed from the start.  children == nullptr: counts[f]
// = the legal actions of its position (0: the game is over).  Otherwise, with offsets [n] the exclusive scan of the
// counts and `total` their sum: child prefix offsets[f] + j = the prefix and its j-th legal action in ascending order
// (children [total][depth + 1]) and keys [total][2] the digest of the child position's planes, written through the
// wavefront's own scratch planes [n][channels][tiles].  err [n] as above.
hipError_t opening_expand_launch(const OpeningGames& og, int n, const int32_t* frontier, int depth, int max_moves,
                                 int32_t* counts, const int32_t* offsets, int total, int32_t* children, uint64_t* keys,
                                 float* planes, int32_t* err, hipStream_t stream);

}  // namespace nz
