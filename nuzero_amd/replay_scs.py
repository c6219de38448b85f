"""Compact replay buffer for SCS games: a position is stored as the game state it was, and the training batch is
rendered inside the gather kernel (C ABI nz_scs_replay_*, nuzero_amd/csrc/scs_replay.hip).

`DeviceReplayBuffer` keeps one dense row per position -- the state image and the policy over all actions: 10.7 KB on a
5x5 board, 42.8 KB on 10x10 -- and allocates window x MAX_MOVES of them.  `ScsReplayBuffer` has the same surface and the
same contents bit for bit (tests/test_gpu_scs_replay_compact.py), but a slot is a self-contained record of 1.5 to 4 KB:
the rules' state, the game's own map, the root's child list, the value and the game index.  A finished round is saved by
two launches, whatever the games' lengths: one replays every game from its recorded actions and checks every action
against the legal mask before it is stepped, the other replays again and writes the records.

Order, eviction, shuffle, sampling and bucketing are `ReplayIndex`'s, unchanged: the same seeds give the same batches.
"""
from ctypes import byref, c_int32, c_void_p
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._lib import lib
from .replay_device import Batch, ReplayIndex

_FORMAT = "nuzero_amd.scs_replay.1"
_DESC_FIELDS = ("terrain", "vp", "units", "arrival")


def _scs_desc(cfg):
    """nz_scs_desc of a game config (or of a checkpoint's copy of one) and the arrays it points into."""
    keep = (np.ascontiguousarray(cfg.terrain, np.float32), np.ascontiguousarray(cfg.vp, np.int32),
            np.ascontiguousarray(cfg.units, np.int32), np.ascontiguousarray(cfg.arrival, np.uint8))
    d = _lib.ScsDesc(rows=cfg.rows, cols=cfg.cols, turns=cfg.turns, stacking=cfg.stacking, terrain=keep[0].ctypes.data,
                     n_vp=(c_int32 * 2)(*cfg.n_vp), vp=keep[1].ctypes.data, n_units=len(keep[2]), units=keep[2].ctypes.data,
                     arrival=keep[3].ctypes.data)
    return d, keep


def record_bytes(config, max_children=0):
    """Bytes of one position of `config`'s board shape with `max_children` child entries (0: the config's own bound,
    rounded as the search engine rounds it).  Host code: needs no GPU."""
    d, _keep = _scs_desc(config)
    n = int(lib.nz_scs_replay_record_bytes(byref(d), int(max_children)))
    if n < 0:
        raise _lib.NzError(_lib.NZ_ERR_ARG, (lib.nz_scs_replay_last_error(None) or b"").decode())
    return n


class ScsReplayBuffer:
    def __init__(self, window_size, batch_size, config, max_game_length, max_children, device=0):
        """`window_size` in games and `batch_size` as the reference's constructor; `config` (ScsGameConfig or a path)
        gives the board shape every game of the buffer must have; `max_game_length` bounds the positions of one game
        (capacity = window x that) and `max_children` the root's children: the engine's MAX_MOVES and MAX_CHILDREN."""
        from .scs import ScsGameConfig
        if not torch.cuda.is_available():
            raise RuntimeError("nuzero_amd needs a ROCm GPU; there is no CPU fallback")
        cfg = config if isinstance(config, ScsGameConfig) else ScsGameConfig(config)
        self.window_size, self.batch_size = int(window_size), int(batch_size)
        self.state_shape = (cfg.channels, cfg.rows, cfg.cols)
        self.num_actions = int(cfg.num_actions)
        self.max_children = int(max_children)
        self.device = torch.device("cuda", device)
        self.capacity = self.window_size * int(max_game_length)
        self.index = ReplayIndex(window_size, self.capacity)
        self.step_to_size_map = {}
        self.allow_partial_loading = True
        self._descs = {}                     # game_index -> the registered description's arrays (checkpoints)
        self._h = c_void_p(0)
        st = lib.nz_scs_replay_create(byref(self._h), self.capacity, self.max_children, cfg.channels, cfg.rows, cfg.cols,
                                      self.num_actions, int(device))
        if st != _lib.NZ_OK:
            raise _lib.NzError(st, (lib.nz_scs_replay_last_error(None) or b"").decode())
        rb = c_int32(0)
        self._check(lib.nz_scs_replay_dims(self._h, None, byref(rb), None, None))
        self.bytes_per_position = int(rb.value)

    # ---- plumbing ------------------------------------------------------------------------------------------
    def _check(self, st):
        if st != _lib.NZ_OK:
            raise _lib.NzError(st, (lib.nz_scs_replay_last_error(self._h) or b"").decode())

    def _stream(self):
        return c_void_p(torch.cuda.current_stream().cuda_stream)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.nz_scs_replay_destroy(self._h)
            self._h = c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self):
        self._check(lib.nz_scs_replay_check(self._h, self._stream()))

    def register(self, game_index, config):
        """The game description batches of `game_index` are rendered with.  Raises NzError for a description of another
        board shape, one whose positions can have more children than the records hold, or an index that already has a
        different description."""
        d, keep = _scs_desc(config)
        self._check(lib.nz_scs_replay_register(self._h, int(game_index), byref(d)))
        if int(game_index) not in self._descs:
            self._descs[int(game_index)] = dict(
                rows=int(config.rows), cols=int(config.cols), turns=int(config.turns), stacking=int(config.stacking),
                n_vp=[int(config.n_vp[0]), int(config.n_vp[1])], **{k: torch.from_numpy(a.copy()) for k, a in zip(_DESC_FIELDS, keep)})

    # ---- filling ---------------------------------------------------------------------------------------------
    def save_scs_games(self, selfplay, result_device, game_index, n_games=None):
        """The (first `n_games`) games of a finished SCS round (nuzero_amd.scs.ScsSelfPlay), as
        DeviceReplayBuffer.save_scs_games takes them.  `selfplay.cfg` is registered under `game_index` on first use.
        Every game is first replayed and checked (NzError naming game and move, the buffer untouched); then one launch
        writes the records.  Only the games' lengths visit the host (the order logic needs them)."""
        r = result_device
        cfg, G = selfplay.cfg, int(r["lengths"].shape[0])
        self.register(game_index, cfg)
        n_keep = G if n_games is None else int(n_games)
        lengths = r["lengths"].cpu().numpy()
        i32 = lambda t: t.to(device=self.device, dtype=torch.int32).contiguous()
        actions, lengths_d, outcomes = i32(r["actions"]), i32(r["lengths"]), i32(r["outcomes"])
        terrain = vp = None
        if cfg.per_game:                                      # every game is replayed on its own map
            terrain, vp = selfplay.game_maps_device()
            assert terrain.shape[0] >= n_keep and terrain.is_contiguous() and vp.is_contiguous()
        ptr = lambda t: c_void_p(t.data_ptr()) if t is not None else None
        M = int(actions.shape[1])
        self._check(lib.nz_scs_replay_check_games(self._h, int(game_index), n_keep, ptr(actions), M, ptr(lengths_d),
                                                  ptr(outcomes), ptr(terrain), ptr(vp), self._stream()))
        dst = self.index.save_games(lengths[:n_keep], game_index)
        dst_d = torch.from_numpy(np.ascontiguousarray(dst)).to(self.device)
        ca, cv, nc = i32(r["child_action"]), i32(r["child_visit"]), i32(r["n_children"])
        self._check(lib.nz_scs_replay_save(self._h, int(game_index), n_keep, ptr(actions), M, ptr(lengths_d), ptr(outcomes),
                                           ptr(terrain), ptr(vp), ptr(ca), ptr(cv), ptr(nc), int(ca.shape[-1]), ptr(dst_d),
                                           int(dst.shape[1]), self._stream()))
        return lengths[:n_keep]

    def save_game(self, game, game_index):
        raise NotImplementedError("ScsReplayBuffer stores game states, and a host record object holds state images, which "
                                  "cannot be turned back into states: save rounds with save_scs_games, or use "
                                  "nuzero_amd.replay_device.DeviceReplayBuffer for record objects")

    # ---- reading -----------------------------------------------------------------------------------------------
    def _gather(self, slots, group_by_game=False):
        keys = counts = None
        if group_by_game:
            slots, keys, counts = self.index.bucket(slots)
        slots_d = torch.from_numpy(np.ascontiguousarray(slots, dtype=np.int64)).to(self.device)
        B = int(slots_d.numel())
        states = torch.empty((B,) + self.state_shape, dtype=torch.float32, device=self.device)
        policies = torch.empty((B, self.num_actions), dtype=torch.float32, device=self.device)
        values = torch.empty((B,), dtype=torch.float32, device=self.device)
        gi = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._check(lib.nz_scs_replay_gather(self._h, c_void_p(slots_d.data_ptr()), B, c_void_p(states.data_ptr()),
                                             c_void_p(policies.data_ptr()), c_void_p(values.data_ptr()),
                                             c_void_p(gi.data_ptr()), self._stream()))
        return Batch(states, policies, values, gi, keys, counts)

    def shuffle(self):
        self.index.shuffle()

    def get_slice(self, start_index, last_index, group_by_game=False):
        return self._gather(self.index.get_slice(start_index, last_index), group_by_game)

    def get_sample(self, batch_size, replace, probs, group_by_game=False):
        return self._gather(self.index.get_sample(batch_size, replace, probs), group_by_game)

    def get_buffer(self):
        """The whole buffer in the reference's list-of-tuples form (compatibility; renders and copies everything)."""
        return self._gather(self.index.seq).as_list()

    def len(self):
        return len(self.index)

    def played_games(self):
        return self.index.n_games

    # ---- checkpoints -------------------------------------------------------------------------------------------
    def save_to_file(self, file_path, step):
        """The reference's layout (ReplayBuffer.py:64-79), rendered through the gather: the host ReplayBuffer and
        DeviceReplayBuffer load it.  This class cannot (see load_from_file); its own checkpoint is save_compact."""
        self.step_to_size_map[step] = (self.len(), self.played_games())
        if self.index.full:
            self.allow_partial_loading = False
        torch.save({"buffer": self.get_buffer(), "map": self.step_to_size_map,
                    "partial_loading": self.allow_partial_loading}, file_path)

    def load_from_file(self, file_path, step):
        raise NotImplementedError("a checkpoint in the reference's layout holds state images, which cannot be turned back "
                                  "into game states: load it into nuzero_amd.replay_device.DeviceReplayBuffer, or use "
                                  "save_compact / load_compact for this class")

    def save_compact(self, file_path):
        """The buffer's own checkpoint: the raw records of the slots in use, the index (order, games, window state,
        game index per slot), the step map and the registered descriptions."""
        n = len(self.index)
        raw = torch.empty((n, self.bytes_per_position), dtype=torch.uint8, device=self.device)
        self._check(lib.nz_scs_replay_export_slots(self._h, n, c_void_p(raw.data_ptr()), self._stream()))
        self.check()
        torch.save({"format": _FORMAT, "record_bytes": self.bytes_per_position, "max_children": self.max_children,
                    "state_shape": list(self.state_shape), "records": raw.cpu(),
                    "seq": torch.from_numpy(self.index.seq.copy()), "n_games": int(self.index.n_games),
                    "full": bool(self.index.full),
                    "slot_game_index": torch.from_numpy(self.index.slot_game_index[:n].copy()),
                    "map": self.step_to_size_map, "partial_loading": self.allow_partial_loading,
                    "descs": self._descs}, file_path)

    def load_compact(self, file_path):
        ck = torch.load(file_path, weights_only=True)
        if ck.get("format") != _FORMAT:
            raise ValueError(f"{file_path} is not a compact SCS replay checkpoint")
        if int(ck["record_bytes"]) != self.bytes_per_position or list(ck["state_shape"]) != list(self.state_shape):
            raise ValueError(f"the checkpoint's records are {ck['record_bytes']} bytes for images {ck['state_shape']}, this "
                             f"buffer's {self.bytes_per_position} for {list(self.state_shape)}")
        raw = ck["records"].contiguous()
        n = int(raw.shape[0])
        if n > self.capacity:
            raise ValueError(f"the checkpoint holds {n} positions, capacity is {self.capacity}")
        for gi, d in ck["descs"].items():
            self.register(gi, SimpleNamespace(**{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()}))
        raw_d = raw.to(self.device)
        self._check(lib.nz_scs_replay_import_slots(self._h, n, c_void_p(raw_d.data_ptr()), self._stream()))
        self.index = ReplayIndex(self.window_size, self.capacity)
        self.index.seq = ck["seq"].numpy().astype(np.int64)
        self.index.n_games, self.index.full = int(ck["n_games"]), bool(ck["full"])
        self.index.slot_game_index = ck["slot_game_index"].numpy().astype(np.int32)
        self.step_to_size_map, self.allow_partial_loading = ck["map"], ck["partial_loading"]
        self.check()
