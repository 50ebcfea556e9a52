"""Device-resident training database -- host mirror of the reference's `Database`
(DAgger/utils/database.py:9-315; Behavior_Cloning/utils/database.py is the same file) over the C-ABI of
include/nmpc_dataset.h.

Same surface and semantics with the rows in HBM: `append` (ring buffer of `limit` rows, statistics
refreshed after every append), `calc_input_mean_std`, `get_database_mean_std`, `set_goal_type`,
`set_normalize_input`, `__len__`, `save_as_npz` / `load_from_npz` (the reference's file schema).  Instead of
one `(x, y)` item per `__getitem__` call, `batch(idx)` assembles a whole normalised batch on the device --
idx typically comes from `policy.weighted_sample` -- ready for `DevicePolicy.train_step`.

Rows are stored in fp32 (what the rollout kernels produce and the network consumes); the statistics are
float64 like numpy's.  Indices are PHYSICAL ring positions, as in the reference (`self.states[index]`).

Beside the reference's four fields every row carries a sampling weight (`weights`, fp32 [limit]: the out-of-distribution
weight `collect.collect_rollouts` computed for it, 1 where none was given).  It rides the ring with the row, so after any
number of appends and wraps `weights[i]` is the weight of physical row i -- what the weighted sampler of
`DevicePolicy.train_epoch` needs.  It is no field of the file schema: npz files are the reference's."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream

FIELDS = ("states", "vc_goals", "cc_goals", "actions")
STATS_MAX_COLS = 64                                       # the widest table nmpc_column_stats takes in one call (include/nmpc_dataset.h)


def column_stats(table: torch.Tensor, rows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """np.mean(table[:rows], axis=0), np.std(table[:rows], axis=0) in float64 on the device."""
    lib = _lib.load()
    assert table.is_cuda and table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 2
    rows = table.shape[0] if rows is None else int(rows)
    cols = table.shape[1]
    if cols > STATS_MAX_COLS:
        # a table wider than the kernel takes (the wide rows of a history policy): the statistics of a column depend on that column
        # alone, so the table goes through in pieces of columns, each a dense copy -- runs of 44 first, the kernel's state width
        widths = [44] * (cols // 44)
        rest = cols - sum(widths)
        widths += [STATS_MAX_COLS] * (rest // STATS_MAX_COLS) + [rest % STATS_MAX_COLS] * (rest % STATS_MAX_COLS > 0)
        pieces, c0 = [], 0
        for w in widths:
            pieces.append(column_stats(table[:rows, c0:c0 + w].contiguous()))
            c0 += w
        return torch.cat([p[0] for p in pieces]), torch.cat([p[1] for p in pieces])
    out = torch.empty(2, cols, dtype=torch.float64, device=table.device)
    scratch = torch.empty(lib.nmpc_column_stats_scratch(cols), dtype=torch.float64, device=table.device)
    _lib.check(lib.nmpc_column_stats(ptr(table), rows, cols, ptr(out[0]), ptr(out[1]), ptr(scratch), stream(table.device)),
               None, "nmpc_column_stats", "dataset")
    return out[0], out[1]


class DeviceDatabase:
    def __init__(self, limit: int, n_state: int = 44, n_action: int = 12, n_vc_goal: int = 3, n_cc_goal: int = 8,
                 norm_input: bool = True, goal_type: str = "vc", device="cuda:0"):
        assert goal_type in ("vc", "cc"), "Goal type can only be vc or cc"
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceDatabase needs a HIP device: there is no CPU path")
        _lib.load()
        self.device = torch.device(device)
        self.limit, self.length, self.start = int(limit), 0, 0
        self.widths = {"states": n_state, "vc_goals": n_vc_goal, "cc_goals": n_cc_goal, "actions": n_action}
        self.tables = {f: torch.zeros(self.limit, w, dtype=torch.float32, device=self.device) for f, w in self.widths.items()}
        self.weights = torch.zeros(self.limit, dtype=torch.float32, device=self.device)
        self.has = {"vc_goals": False, "cc_goals": False}
        self.norm_input, self.goal_type = bool(norm_input), goal_type
        self.states_mean = self.states_std = None          # float64 device vectors
        self.cc_goals_mean = self.cc_goals_std = None
        self.vc_goals_mean, self.vc_goals_std = 0.0, 1.0   # database.py:240-243: 'vc' goals are not normalised

    def __len__(self):
        return self.length

    def set_normalize_input(self, value: bool):
        self.norm_input = bool(value)

    def set_goal_type(self, value: str):
        assert value in ("vc", "cc"), "Goal type can only be vc or cc"
        self.goal_type = value

    # ------------------------------------------------------------------ aggregation
    def append(self, states, actions, vc_goals=None, cc_goals=None, weights=None):
        """database.py:105-154.  Arguments: device (or host) arrays [n, width]; weights: [n] sampling weights of the rows
        (None: ones)."""
        if vc_goals is None and cc_goals is None:
            raise ValueError("both vc_goals and cc_goals cant be empty!")
        lib = _lib.load()
        given = {"states": states, "actions": actions, "vc_goals": vc_goals, "cc_goals": cc_goals}
        n = None
        for f, a in list(given.items()):
            if a is None:
                continue
            a = torch.as_tensor(a, dtype=torch.float32, device=self.device).contiguous()
            if a.dim() != 2 or a.shape[1] != self.widths[f] or (n is not None and a.shape[0] != n):
                raise ValueError(f"{f}: expected [{n if n is not None else 'n'}, {self.widths[f]}], got {tuple(a.shape)}")
            n = a.shape[0]
            given[f] = a
        if weights is None:
            weights = torch.ones(n, dtype=torch.float32, device=self.device)
        weights = torch.as_tensor(weights, dtype=torch.float32, device=self.device).contiguous()
        if weights.shape != (n,):
            raise ValueError(f"weights: expected [{n}], got {tuple(weights.shape)}")
        first_slot = (self.start + self.length) % self.limit
        _lib.check(lib.nmpc_ring_append(ptr(weights), 1, n, ptr(self.weights), self.limit, first_slot, stream(self.device)),
                   None, "nmpc_ring_append", "dataset")
        for f, a in given.items():
            if a is None:
                continue
            _lib.check(lib.nmpc_ring_append(ptr(a), a.shape[1], n, ptr(self.tables[f]), self.limit, first_slot,
                                            stream(self.device)), None, "nmpc_ring_append", "dataset")
            if f in self.has:
                self.has[f] = True
        grow = min(n, self.limit - self.length)             # room first, then the start moves (:124-131)
        self.length += grow
        self.start = (self.start + n - grow) % self.limit
        self.calc_input_mean_std()

    def calc_input_mean_std(self):
        """database.py:208-255: statistics over the physical rows [0, length)."""
        if self.length == 0:
            return
        self.states_mean, self.states_std = column_stats(self.tables["states"], self.length)
        if self.has["cc_goals"]:
            self.cc_goals_mean, self.cc_goals_std = column_stats(self.tables["cc_goals"], self.length)

    def get_database_mean_std(self):
        """[states_mean, states_std, goal_mean, goal_std] (numpy float64) or None -- database.py:257-271."""
        if not self.norm_input:
            return None
        out = [self.states_mean.cpu().numpy(), self.states_std.cpu().numpy()]
        if self.goal_type == "vc":
            return out + [self.vc_goals_mean, self.vc_goals_std]
        return out + [self.cc_goals_mean.cpu().numpy(), self.cc_goals_std.cpu().numpy()]

    # ------------------------------------------------------------------ batches
    def batch_source(self) -> _lib.NmpcBatchSource:
        """What a batch is assembled from under the current goal type and normalisation switch (nmpc_batch_source of
        include/nmpc_policy.h): the tables and statistics `batch` reads, and `DevicePolicy.train_epoch` with it.  The
        pointers are the database's own tensors: use it before the next append."""
        if self.length == 0:
            raise IndexError("the database is empty")
        goal_field = "vc_goals" if self.goal_type == "vc" else "cc_goals"
        if not self.has[goal_field]:
            raise ValueError(f"no {goal_field} were appended")
        s_mean = s_std = g_mean = g_std = None
        if self.norm_input:
            s_mean, s_std = self.states_mean, self.states_std
            if self.goal_type == "cc":
                g_mean, g_std = self.cc_goals_mean, self.cc_goals_std
        return _lib.NmpcBatchSource(ptr(self.tables["states"]), self.widths["states"], ptr(s_mean), ptr(s_std), 1,
                                    ptr(self.tables[goal_field]), self.widths[goal_field], ptr(g_mean), ptr(g_std),
                                    ptr(self.tables["actions"]), self.widths["actions"], self.length)

    def batch(self, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x[i] = hstack(state_norm, goal)[idx[i]], y[i] = actions[idx[i]] as fp32 (database.py:54-84 and
        the `.float()` of train_locosafedagger.py:95) for int32 device indices."""
        lib = _lib.load()
        assert idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.dim() == 1
        s = self.batch_source()
        x = torch.empty(idx.numel(), s.n_state + s.n_goal, dtype=torch.float32, device=self.device)
        y = torch.empty(idx.numel(), s.n_action, dtype=torch.float32, device=self.device)
        _lib.check(lib.nmpc_assemble_batch(s.states, s.n_state, s.s_mean, s.s_std, s.s_first, s.goals, s.n_goal, s.g_mean,
                                           s.g_std, s.actions, s.n_action, s.n_rows, ptr(idx), idx.numel(),
                                           ptr(x), ptr(y), stream(self.device)), None, "nmpc_assemble_batch", "dataset")
        return x, y

    # ------------------------------------------------------------------ files (npz first)
    def save_as_npz(self, filename: str):
        """database.py:273-282: keys states, vc_goals, cc_goals, actions -- float64 arrays [length, width]."""
        np.savez(filename, **{f: self.tables[f][:self.length].cpu().numpy().astype(np.float64) for f in FIELDS})

    def load_from_npz(self, filename: str):
        """database.py:284-315: replaces the contents, then recomputes the statistics."""
        data = np.load(filename)
        for f in FIELDS:
            if f not in data:
                raise ValueError(f"Missing field '{f}' in NPZ file.")
        n = len(data["states"])
        if n > self.limit:
            raise ValueError(f"{n} rows do not fit limit={self.limit}")
        for f in FIELDS:
            a = np.asarray(data[f], dtype=np.float32)
            if a.shape != (n, self.widths[f]):
                raise ValueError(f"{f}: expected {(n, self.widths[f])}, got {a.shape}")
            self.tables[f][:n] = torch.from_numpy(a).to(self.device)
        self.weights[:n] = 1.0
        self.has = {"vc_goals": True, "cc_goals": True}
        self.length, self.start = n, 0
        self.calc_input_mean_std()
