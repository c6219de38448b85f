"""Tic-Tac-Toe positions as the engine's bitboard words, for evaluation from given positions (C ABI nz_engine_reset_to,
nz_engine_match_play_from, nz_engine_policy_actions): the openings of k plies, the 4,520 reachable non-terminal
positions, and perfect play on them.  Plain numpy; nothing here needs a GPU.

A position is one uint32: player-one stones in bits 0-8, player-two stones in bits 16-24 (cell = row * 3 + col).  It is
*playable* when no other bit is set, the two stone sets are disjoint, stones(p1) - stones(p2) is 0 or 1, neither side
has a line and at least one cell is empty; how it arose is not checked.  Positions are listed in
ascending order of their base-3 code (`ttt_code`: cell a has weight 3^a, 1 = player one, 2 = player two), the key of the
table evaluator.
"""
import numpy as np

N_CODES = 3 ** 9
_LINES = (0o007, 0o070, 0o700, 0o111, 0o222, 0o444, 0o421, 0o124)
_BOARD_BITS = 0x01FF01FF


def _line(m):
    return any((m & l) == l for l in _LINES)


def _stones(m):
    return bin(m).count("1")


def ttt_code(board):
    """The base-3 position code of a bitboard word: sum over cells of (1 | 2) * 3^cell."""
    board = int(board)
    return sum((((board >> a) & 1) + 2 * ((board >> (16 + a)) & 1)) * 3 ** a for a in range(9))


def is_playable(board):
    """(True, None), or (False, reason): the first condition the position fails, in the words the library refuses it
    with."""
    b = int(board)
    if b < 0 or b & ~_BOARD_BITS:
        return False, "a bit outside the stone sets (bits 0-8 and 16-24) is set"
    p1, p2 = b & 0x1FF, (b >> 16) & 0x1FF
    if p1 & p2:
        return False, "a cell holds a stone of both players"
    if _stones(p1) - _stones(p2) not in (0, 1):
        return False, "stones(p1) - stones(p2) is neither 0 nor 1"
    if _line(p1) or _line(p2):
        return False, "a side has a line: the game is over"
    if (p1 | p2) == 0x1FF:
        return False, "no cell is empty"
    return True, None


def board_from_actions(actions):
    """The position after `actions` (cell indices, player one first) from the empty board.  Refuses an occupied cell
    and a move after the game has ended."""
    b = 0
    for ply, a in enumerate(actions):
        a = int(a)
        if not 0 <= a < 9:
            raise ValueError(f"action {a} at ply {ply}: cells are 0 .. 8")
        if ((b | (b >> 16)) >> a) & 1:
            raise ValueError(f"action {a} at ply {ply}: the cell is taken")
        if _terminal(b):
            raise ValueError(f"action {a} at ply {ply}: the game is over")
        b |= (1 << a) << (16 if ply % 2 else 0)
    return np.uint32(b)


def _terminal(b):
    p1, p2 = b & 0x1FF, (b >> 16) & 0x1FF
    return _line(p1) or _line(p2) or (p1 | p2) == 0x1FF


def _children(b):
    shift = 16 if _stones(b) % 2 else 0
    taken = b | (b >> 16)
    return [(a, b | ((1 << a) << shift)) for a in range(9) if not (taken >> a) & 1]


_memo = {}


def _reachable():
    """Every position reachable from the empty board by legal play (terminal ones included), by stone count."""
    if "reachable" not in _memo:
        levels, level = [], {0}
        for _ in range(10):
            levels.append(sorted(level, key=ttt_code))
            level = {c for b in level if not _terminal(b) for _, c in _children(b)}
        _memo["reachable"] = levels
    return _memo["reachable"]


def openings(plies):
    """The playable positions with exactly `plies` stones that legal play reaches from the empty board: uint32, in
    ascending order of ttt_code.  (1, 9, 72, 252, 756, 1140, 1372, 696, 222 positions for 0 .. 8 plies.)"""
    plies = int(plies)
    if not 0 <= plies <= 8:
        raise ValueError(f"openings of {plies} plies: a playable position holds 0 .. 8 stones")
    return np.array([b for b in _reachable()[plies] if not _terminal(b)], np.uint32)


def reachable_nonterminal():
    """All 4,520 reachable playable positions: uint32, in ascending order of ttt_code."""
    every = [b for level in _reachable()[:9] for b in level if not _terminal(b)]
    return np.array(sorted(every, key=ttt_code), np.uint32)


def perfect_play():
    """(values int8 [3^9], masks int32 [3^9]) by position code, by plain minimax with a memo: the game-theoretic value
    from player 1's view (+1 player 1 wins, 0 draw, -1 player 2 wins; a terminal position's own value) and the 9-bit
    mask of the moves that keep it (0 for a terminal position).  Codes no legal play reaches hold 0 / 0."""
    if "perfect" not in _memo:
        values, masks = np.zeros(N_CODES, np.int8), np.zeros(N_CODES, np.int32)
        value_of = {}

        def solve(b):
            if b in value_of:
                return value_of[b]
            p1, p2 = b & 0x1FF, (b >> 16) & 0x1FF
            if _line(p1) or _line(p2) or (p1 | p2) == 0x1FF:
                v, mask = (1 if _line(p1) else -1 if _line(p2) else 0), 0
            else:
                kids = [(a, solve(c)) for a, c in _children(b)]
                v = max(x for _, x in kids) if _stones(b) % 2 == 0 else min(x for _, x in kids)
                mask = sum(1 << a for a, x in kids if x == v)
            value_of[b] = v
            code = ttt_code(b)
            values[code], masks[code] = v, mask
            return v
        solve(0)
        values.setflags(write=False)
        masks.setflags(write=False)
        _memo["perfect"] = (values, masks)
    return _memo["perfect"]


def check_start_boards(boards, same_ply=False):
    """What the library refuses of a list of start positions, refused here before any GPU call with the same words:
    the first unplayable board, and (same_ply) boards that do not all hold the same number of stones.  Returns the
    boards as a contiguous uint32 array."""
    raw = [int(b) for b in np.asarray(boards).reshape(-1)]
    for i, b in enumerate(raw):
        ok, why = is_playable(b)
        if not ok:
            raise ValueError(f"start board {i} (0x{b & 0xFFFFFFFF:08x}) is not playable: {why}")
    if same_ply:
        for i, b in enumerate(raw):
            if _stones(b) != _stones(raw[0]):
                raise ValueError(f"start boards 0 and {i} hold {_stones(raw[0])} and {_stones(b)} stones: every match "
                                 "of a round starts at the same ply")
    return np.ascontiguousarray(np.array(raw, np.uint32))
