"""Test infrastructure of the Tic-Tac-Toe matches and searches from given positions (nz_engine_reset_to,
nz_engine_match_play_from, nz_engine_policy_actions): the oracle game stepped through a position's stones, an oracle match
and an oracle search that start there, and a walk and a minimax over oracle/ttt.py that share nothing with
nuzero_amd/ttt_positions.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from ttt_match_ref import make_agent, random_table, search_cfg   # noqa: E402,F401


def cells_of(board):
    """The nine cells (0 empty, 1 player one, 2 player two) of a bitboard word."""
    board = int(board)
    return [((board >> a) & 1) + 2 * ((board >> (16 + a)) & 1) for a in range(9)]


def board_of(game):
    """The bitboard word of an oracle game."""
    return sum((1 << a) << (0 if c == 1 else 16) for a, c in enumerate(game.board) if c)


def game_at(board):
    """oracle.ttt.TicTacToe stepped through the position's stones, the players alternating (each side's stones in
    ascending cell order: a position does not say how it arose)."""
    from oracle import ttt as ottt
    cells = cells_of(board)
    mine = {p: [a for a, c in enumerate(cells) if c == p] for p in (1, 2)}
    assert len(mine[1]) - len(mine[2]) in (0, 1), hex(int(board))
    game = ottt.TicTacToe()
    for ply in range(len(mine[1]) + len(mine[2])):
        assert not game.is_terminal()
        game.step_index(mine[1 + ply % 2][ply // 2])
    assert game.board == cells and not game.is_terminal()
    return game


def oracle_match_from(board, spec1, table1, spec2, table2):
    """ttt_match_ref.oracle_match from a start position: side 1 still moves for player 1.  The record is by absolute
    ply: `actions` is the list played from the position, `first_ply` its stone count."""
    from oracle.agents import play_match
    game = game_at(board)
    k = game.length
    agents = [make_agent(spec1, table1), make_agent(spec2, table2)]
    actions = [int(a) for a in play_match(game, agents[0], agents[1])]
    out = {"actions": actions, "first_ply": k, "length": int(game.length), "terminal_value": int(game.terminal_value),
           "sides": []}
    for i, (spec, ag) in enumerate(zip((spec1, spec2), agents)):
        d = {}
        if spec[0] != "mcts":
            plies = [p for p in range(k, k + len(actions)) if p % 2 == i]
            assert len(plies) == len(ag.actions) == len(ag.n_legal)
            a9, n9 = [-1] * 9, [0] * 9
            for ply, a, n in zip(plies, ag.actions, ag.n_legal):
                a9[ply], n9[ply] = a, n
            d.update(agent_actions=a9, agent_n_legal=n9)
        if spec[0] == "random":
            st = ag.rs.get_state()
            d.update(keys=np.asarray(st[1], np.uint32), pos=int(st[2]))
        out["sides"].append(d)
    return out


def expected_record_from(games):
    """What nz_engine_match_play_from must return for these oracle games: actions [N, 9] by absolute ply (-1 before the
    start and past the end), lengths (stone counts of the final positions), outcomes and the 4-word tally."""
    n = len(games)
    actions = np.full((n, 9), -1, np.int32)
    for i, g in enumerate(games):
        actions[i, g["first_ply"]:g["first_ply"] + len(g["actions"])] = g["actions"]
    lengths = np.array([g["length"] for g in games], np.int32)
    outcomes = np.array([g["terminal_value"] for g in games], np.int32)
    tally = (int((outcomes > 0).sum()), int((outcomes < 0).sum()), int((outcomes == 0).sum()), 0)
    return actions, lengths, outcomes, tally


def oracle_search_at(board, cfg, evaluator):
    """One evaluation search from a fresh root at the position (MctsAgentRef.new_game, then choose_action): the chosen
    action, the root children's visit counts by action [9], their number, and what the move leaves: (terminal?,
    terminal value)."""
    from oracle.search import Explorer, Node
    game = game_at(board)
    root = Node(0)
    action, _, _ = Explorer(cfg, False).run_mcts(game, evaluator, root)
    visits = np.zeros(9, np.int32)
    for c in root.children:
        visits[c.action] = c.visit_count
    game.step_index(action)
    return int(action), visits, len(root.children), bool(game.is_terminal()), int(game.terminal_value)


def walk_positions():
    """{code: oracle game} of every position legal play reaches from the empty board (terminal ones included), by a walk
    over oracle.ttt.TicTacToe alone."""
    from oracle import ttt as ottt
    seen, stack = {}, [ottt.TicTacToe()]
    while stack:
        g = stack.pop()
        if g.code() in seen:
            continue
        seen[g.code()] = g
        if g.is_terminal():
            continue
        for a in range(9):
            if g.board[a] == 0:
                h = g.shallow_clone()
                h.step_index(a)
                stack.append(h)
    return seen


def minimax_on_the_oracle():
    """{code: (value for player 1, 9-bit mask of the moves that keep it)} for every reachable position, by minimax over
    oracle.ttt.TicTacToe."""
    from oracle import ttt as ottt
    memo = {}

    def solve(g):
        code = g.code()
        if code in memo:
            return memo[code][0]
        if g.is_terminal():
            memo[code] = (int(g.get_terminal_value()), 0)
            return memo[code][0]
        kids = []
        for a in range(9):
            if g.board[a] == 0:
                h = g.shallow_clone()
                h.step_index(a)
                kids.append((a, solve(h)))
        best = max(v for _, v in kids) if g.get_current_player() == 1 else min(v for _, v in kids)
        memo[code] = (best, sum(1 << a for a, v in kids if v == best))
        return best
    solve(ottt.TicTacToe())
    return memo


def images_of(boards):
    """float32 [N, 2, 3, 3] network inputs of bitboard words (player-one plane, player-two plane)."""
    x = np.zeros((len(boards), 2, 9), np.float32)
    for i, b in enumerate(boards):
        for a, c in enumerate(cells_of(b)):
            if c:
                x[i, c - 1, a] = 1.0
    return x.reshape(-1, 2, 3, 3)


def gpu_table(engine):
    """The engine's own network on every position code -> a [3^9, 10] table the oracle can read."""
    codes = np.arange(3 ** 9)
    cells = (codes[:, None] // 3 ** np.arange(9)[None, :]) % 3
    x = np.stack([cells == 1, cells == 2], 1).astype(np.float32).reshape(-1, 2, 3, 3)
    _, value, probs = engine.net_forward(x)
    t = np.zeros((3 ** 9, 10), np.float32)
    t[:, :9] = probs.cpu().numpy()
    t[:, 9] = value.cpu().numpy()
    return t
