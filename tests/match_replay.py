"""Test infrastructure: replay an SCS evaluation match on the CPU oracle with the two DEVICE agents' own evaluations.

`oracle.agents.play_match` (Tester.py:62-118) is played with two evaluators, one per agent; each finds the evaluation
of the position it is asked about -- by `scs_replay.image_mix_digest` of the position's planes -- in ONE agent's
recorded (digest, probs, value) list (ScsSelfPlay.records() after a match on the persistent route, cache hits
included).  A position that is not in the list raises: the replay never computes an evaluation itself, so the match it
plays is decided by the device's numbers alone, and every action must then equal the device's.  Each recorded row is
handed out once (the k-th question about a position takes the k-th row recorded for it); `unused()` lists what the
replay never asked for.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from scs_replay import image_mix_digest          # noqa: E402


class MissingEvaluation(LookupError):
    pass


class RecordedEvaluations:
    """evaluator(game) -> (probs, value) out of one agent's recorded list."""

    def __init__(self, digests, probs, values, label=""):
        digests = np.asarray(digests, np.uint64).reshape(-1, 2)
        assert len(digests) == len(probs) == len(values)
        self.probs, self.values, self.label = probs, values, label
        self.rows = {}                          # digest -> the rows recorded for it, in order
        for i, d in enumerate(digests):
            self.rows.setdefault(d.tobytes(), []).append(i)
        self.taken = {k: 0 for k in self.rows}
        self.lookups = 0

    def __call__(self, game):
        key = image_mix_digest(game.state_image()[0]).tobytes()
        rows = self.rows.get(key)
        if rows is None or self.taken[key] >= len(rows):
            raise MissingEvaluation(f"{self.label}: look-up {self.lookups} asks for a position the device agent "
                                    f"{'evaluated fewer times' if rows else 'never evaluated'}")
        i = rows[self.taken[key]]
        self.taken[key] += 1
        self.lookups += 1
        return self.probs[i], self.values[i]

    def unused(self):
        return sorted(i for k, rows in self.rows.items() for i in rows[self.taken[k]:])


class RecordingEvaluator:
    """Wraps evaluator(game) and keeps what RecordedEvaluations reads: the CPU stand-in for ScsSelfPlay.records()."""

    def __init__(self, evaluator):
        self.evaluator, self.digests, self.probs, self.values = evaluator, [], [], []

    def __call__(self, game):
        p, v = self.evaluator(game)
        self.digests.append(image_mix_digest(game.state_image()[0]))
        self.probs.append(np.asarray(p, np.float32).copy())
        self.values.append(np.float32(v))
        return p, v

    def arrays(self):
        return (np.array(self.digests, np.uint64).reshape(-1, 2), np.array(self.probs, np.float32),
                np.array(self.values, np.float32))


def oracle_game(config_path, seed=None, game_map=None):
    """The oracle game of one match; per-game maps: `seed` draws it (np.random.seed(seed); SCS_Game(config)) and
    `game_map` = (terrain [tiles, 3], vp [k, 2]), what the device reports for the match, must be that very map."""
    from oracle.scs import ScsConfig, ScsGame
    cfg = ScsConfig(config_path) if seed is None else ScsConfig(config_path, map_seed=np.random.RandomState(int(seed)))
    if game_map is not None:
        terrain, vp = game_map
        want_t = np.array(cfg.terrain, np.float32).reshape(-1, 3)
        want_v = np.array([p for side in cfg.vp for p in side], np.int32).reshape(-1, 2)
        assert np.array_equal(np.asarray(terrain, np.float32).reshape(-1, 3), want_t), "reported terrain is not the seed's"
        assert np.array_equal(np.asarray(vp, np.int32).reshape(-1, 2), want_v), "reported victory points are not the seed's"
    return ScsGame(cfg)


def replay_match(args):
    """(config path, search config 1, search config 2, records 1, records 2[, seed[, game_map]]) -> dict.  records:
    (digests uint64 [n, 2], probs [n, A], values [n]) of one agent.  Top-level: it can run in a worker process."""
    config_path, search1, search2, rec1, rec2 = args[:5]
    seed = args[5] if len(args) > 5 else None
    game_map = args[6] if len(args) > 6 else None
    from oracle.agents import MctsAgentRef, play_match
    game = oracle_game(config_path, seed, game_map)
    ev1, ev2 = RecordedEvaluations(*rec1, label="agent 1"), RecordedEvaluations(*rec2, label="agent 2")
    actions = play_match(game, MctsAgentRef(search1, ev1), MctsAgentRef(search2, ev2))
    return {"actions": [int(a) for a in actions], "length": int(game.length), "terminal_value": int(game.terminal_value),
            "lookups": (ev1.lookups, ev2.lookups), "recorded": (len(rec1[2]), len(rec2[2])),
            "unused": (ev1.unused(), ev2.unused())}


def replay_matches(jobs, workers=None):
    """Several matches, in worker processes when there is more than one (as scs_replay.replay_games: spawned, at
    most 12)."""
    if len(jobs) <= 1 or workers == 1:
        return [replay_match(j) for j in jobs]
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    workers = workers or min(len(jobs), max(1, (os.cpu_count() or 2) - 1), 12)
    with ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(replay_match, jobs))
