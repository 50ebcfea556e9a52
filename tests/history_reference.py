"""numpy restatement of the observation and action history on the policy input (nmpc_history_push_batch,
nmpc_history_push_actions_batch of include/nmpc_torque.h; helper module, not collected by pytest).

The registers are hist [B, n_obs, 44] (slot 0 the incoming slot, slot h the observed row of h control steps ago) and act
[B, n_act, 12] (slot i the target issued i + 1 control steps before the next one).  Every word of the raw wide row and of the
registers is a copy; the policy input is the database's expression (float32)(((float64)w - mean) / std) on the columns from
s_first on, the goal behind it raw."""
import numpy as np

NS, NU = 44, 12


def width(n_obs, n_act):
    return NS * n_obs + NU * n_act


def normalise(W, s_mean, s_std, s_first):
    """the columns [s_first, n_wide) of float32 W [..., n_wide] through the database's expression, the others raw -> float32"""
    X = np.array(W, np.float32)
    if s_mean is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            X[..., s_first:] = ((W[..., s_first:].astype(np.float64) - np.asarray(s_mean, np.float64)[s_first:])
                                / np.asarray(s_std, np.float64)[s_first:]).astype(np.float32)
    return X


def push(hist, act, goal=None, s_mean=None, s_std=None, s_first=1):
    """the wide row of every robot out of the registers -> (W [B, n_wide], X [B, n_wide + n_goal]); then hist ages IN PLACE, slot
    h + 1 <- slot h from the oldest down, slot 0 keeping its content; act (None or [B, 0, 12]: no actions) is only read"""
    B, n_obs = hist.shape[:2]
    assert hist.dtype == np.float32 and hist.shape[2] == NS
    parts = [hist[:, h] for h in range(n_obs)]
    if act is not None:
        assert act.dtype == np.float32 and act.shape[2] == NU
        parts += [act[:, i] for i in range(act.shape[1])]
    W = np.concatenate(parts, axis=1)
    X = normalise(W, s_mean, s_std, s_first)
    if goal is not None:
        X = np.concatenate([X, np.asarray(goal, np.float32)], axis=1)
    for h in range(n_obs - 1, 0, -1):
        hist[:, h] = hist[:, h - 1]
    return W, X


def push_actions(act, A):
    """the action register moves on by one IN PLACE: slot s <- slot s - 1 from the oldest down, then slot 0 <- A [B, 12]"""
    for s in range(act.shape[1] - 1, 0, -1):
        act[:, s] = act[:, s - 1]
    act[:, 0] = A


def reset(S0, posture, n_obs, n_act):
    """the registers with every slot of robot b holding S0[b] [44] and posture[b] [12]"""
    S0, posture = np.asarray(S0, np.float32), np.asarray(posture, np.float32)
    return np.repeat(S0[:, None], n_obs, axis=1).copy(), np.repeat(posture[:, None], n_act, axis=1).copy()


def chained(O, A, S0, posture, n_obs, n_act):
    """K chained pushes from the reset registers: in step k slot 0 <- O[:, k], push, push_actions(A[:, k])
    -> (W [B, K, n_wide], hist, act afterwards)"""
    hist, act = reset(S0, posture, n_obs, n_act)
    rows = []
    for k in range(O.shape[1]):
        hist[:, 0] = O[:, k]
        rows.append(push(hist, act)[0])
        if n_act:
            push_actions(act, A[:, k])
    return np.stack(rows, axis=1), hist, act


def closed_form(O, A, S0, posture, n_obs, n_act):
    """W[b, k] = [O_k | O_{k-1} | ... | O_{k-n_obs+1} | A_{k-1} | ... | A_{k-n_act}], an entry from before step 0 being the fill"""
    B, K = O.shape[:2]
    W = np.empty((B, K, width(n_obs, n_act)), np.float32)
    for k in range(K):
        for h in range(n_obs):
            W[:, k, NS * h:NS * (h + 1)] = O[:, k - h] if k >= h else S0
        for i in range(n_act):
            j = k - 1 - i
            W[:, k, NS * n_obs + NU * i:NS * n_obs + NU * (i + 1)] = A[:, j] if j >= 0 else posture
    return W
