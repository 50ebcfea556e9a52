"""The rules of nmpc_observed_rows_batch (include/nmpc_torque.h) and nmpc_policy_input_noise_batch (include/nmpc_policy.h) restated
in numpy (helper module, not collected by pytest), on the Philox and the constants of tests/noise_reference.py.  Every operation
below is one IEEE operation on arrays -- numpy fuses nothing -- so the results are the rules' to the bit."""
import numpy as np

from tests.noise_reference import C, N_SLOTS, T_MAX, philox4x32_10, variate

TRAINING_WORD = 1                                          # the fourth counter word of the training draws; the sensor rule has 0


def integer_variate4(c0, c1, c2, c3, seed):
    """t at a full counter (c0, c1, c2, c3): the centred sum of the four 16-bit halves of the two words, int64, |t| <= T_MAX"""
    w0, w1 = philox4x32_10(c0, c1, c2, c3, seed)
    h = np.uint64(0xFFFF)
    return ((w0 & h) + (w0 >> np.uint64(16)) + (w1 & h) + (w1 >> np.uint64(16))).astype(np.int64) - T_MAX


def variate4(c0, c1, c2, c3, seed):
    """g at a full counter, float32: one product"""
    return integer_variate4(c0, c1, c2, c3, seed).astype(np.float32) * C


def observed_rows(S, noise, seed, first_robot, step):
    """S [B, >= 44] float32 -> O [B, 44] float32, the rows as the sensors show them at `step`; noise [>= B, 88] float32 (sigma,
    bias) or None: no table, O is S"""
    S = np.asarray(S, dtype=np.float32)[:, :N_SLOTS]
    if noise is None:
        return S.copy()
    B = S.shape[0]
    sigma, bias = np.asarray(noise, np.float32)[:B, :N_SLOTS], np.asarray(noise, np.float32)[:B, N_SLOTS:]
    robot = ((int(first_robot) + np.arange(B, dtype=object)) % 2 ** 32).astype(np.uint64)
    g = variate(robot[:, None], int(step) % 2 ** 32, np.arange(N_SLOTS)[None, :], seed)
    n = bias.astype(np.float64) + sigma.astype(np.float64) * g.astype(np.float64)
    out = (S.astype(np.float64) + n).astype(np.float32)
    return np.where((sigma != 0) | (bias != 0), out, S)


def input_noise(X, sigma, seed, epoch, first_sample=0, s_std=None, s_first=1):
    """X [B, >= n] float32 under the training rule -> a new array; sigma float32 [n], s_std float64 [>= n] or None"""
    X = np.array(X, dtype=np.float32)
    sigma = np.asarray(sigma, np.float32)
    B, n = X.shape[0], sigma.shape[0]
    sample = ((int(first_sample) + np.arange(B, dtype=object)) % 2 ** 32).astype(np.uint64)
    g = variate4(sample[:, None], int(epoch) % 2 ** 32, np.arange(n)[None, :], TRAINING_WORD, seed)
    nz = sigma.astype(np.float64)[None, :] * g.astype(np.float64)
    if s_std is not None:
        scale = np.ones(n)
        scale[s_first:] = np.asarray(s_std, np.float64)[s_first:n]
        nz = np.where(np.arange(n) >= s_first, nz / scale, nz)
    out = (X[:, :n].astype(np.float64) + nz).astype(np.float32)
    X[:, :n] = np.where(sigma[None, :] != 0, out, X[:, :n])
    return X


def training_sigma(noise):
    """per slot the root mean square over the robots of sqrt(sigma^2 + bias^2), float32 [44]"""
    noise = np.asarray(noise, np.float64)
    return np.sqrt((noise[:, :N_SLOTS] ** 2 + noise[:, N_SLOTS:] ** 2).mean(axis=0)).astype(np.float32)
