"""MI355X-native self-play engine behind NuZero's Gamer / Game / Network_Manager /
ReplayBuffer surface.

Only the self-play hot path lives here: batched MCTS over
thousands of game trees with policy/value inference fused in, as hand-written
HIP kernels for gfx950 reached through the C ABI of include/nuzero_amd.h.
Importing a submodule that needs the shared library raises if it has not been
built (``python -m nuzero_amd.build``); there is no CPU fallback.
"""
__version__ = "0.1"


def __getattr__(name):
    # the evaluation-match front end, imported on first use (it loads the shared library)
    if name in ("ScsMatch", "ScsAgentMatch", "ScsTester", "TttMatch", "TttAgentMatch", "TttTester"):
        from . import tester
        return getattr(tester, name)
    if name == "ScsReplayBuffer":              # the compact SCS replay buffer (it loads the shared library)
        from . import replay_scs
        return replay_scs.ScsReplayBuffer
    if name == "ttt_positions":                # start positions of the Tic-Tac-Toe matches (plain numpy)
        import importlib
        return importlib.import_module(".ttt_positions", __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
