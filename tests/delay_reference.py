"""The delay line of include/nmpc_torque.h (nmpc_contact_set_delays, nmpc_delay_line_batch) restated in numpy, element by element
as the header writes it (helper module, not collected by pytest).  Nothing is computed: every output is a copy of an input, so the
GPU tests compare against it with exact equality."""
import numpy as np


def delay_line(issued, history, delay):
    """issued [B, n_steps, nu], history [B, depth, nu] (slot j: the target issued j + 1 control steps before the next one), delay
    [B] integers (clamped into [0, depth] here as on the device) -> (applied [B, n_steps, nu], the new history [B, depth, nu]):
        d = min(max(delay[b], 0), depth)
        P[b][k]  = k >= d ? I[b][k - d] : H[b][d - 1 - k]
        H'[b][j] = n_steps - 1 - j >= 0 ? I[b][n_steps - 1 - j] : H[b][j - n_steps]"""
    issued, history = np.asarray(issued), np.asarray(history)
    B, n_steps, _ = issued.shape
    depth = history.shape[1]
    applied, new = np.empty_like(issued), np.empty_like(history)
    for b in range(B):
        d = min(max(int(delay[b]), 0), depth)
        for k in range(n_steps):
            applied[b, k] = issued[b, k - d] if k >= d else history[b, d - 1 - k]
        for j in range(depth):
            new[b, j] = issued[b, n_steps - 1 - j] if n_steps - 1 - j >= 0 else history[b, j - n_steps]
    return applied, new
