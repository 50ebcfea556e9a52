"""The rule of nmpc_contact_set_noise / nmpc_observe_noise_batch (include/nmpc_torque.h) restated in numpy (helper module, not
collected by pytest): a Philox-4x32-10 of its own on general counters in uint64 arithmetic, the integer variate, and the float32
and float64 casts exactly where the rule has them.  Every operation below is one IEEE operation on arrays -- numpy fuses
nothing -- so the result is the rule's to the bit."""
import numpy as np

N_SLOTS = 44
M32 = np.uint64(0xFFFFFFFF)
C = np.float32(1.0 / np.sqrt((2.0 ** 32 - 1.0) / 3.0))     # the variance of a sum of four uniforms on 0 .. 65535 is (2^32 - 1) / 3
T_MAX = 131070                                             # the largest |t|: 4 * 65535 / 2


def philox4x32_10(c0, c1, c2, c3, seed):
    """the first two output words of Philox-4x32-10 at counters (c0, c1, c2, c3) -- arrays that broadcast, any integers, taken
    mod 2^32 -- under the key (seed lo, seed hi)"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    seed = int(seed) & (2 ** 64 - 1)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2      # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1


def integer_variate(robot, step, slot, seed):
    """t of the rule: the centred sum of the four 16-bit halves of the two words, an int64 with |t| <= T_MAX"""
    w0, w1 = philox4x32_10(robot, step, slot, 0, seed)
    h = np.uint64(0xFFFF)
    return ((w0 & h) + (w0 >> np.uint64(16)) + (w1 & h) + (w1 >> np.uint64(16))).astype(np.int64) - T_MAX


def variate(robot, step, slot, seed):
    """g of the rule, float32: one product"""
    return integer_variate(robot, step, slot, seed).astype(np.float32) * C


def observe_noise(X, noise, seed, first_robot, step, s_std=None, s_first=1):
    """X [B, >= 44] float32 under the rule -> a new array; noise [>= B, 88] float32 (sigma, bias), s_std float64 [44] or None"""
    X = np.array(X, dtype=np.float32)
    B = X.shape[0]
    sigma, bias = np.asarray(noise, np.float32)[:B, :N_SLOTS], np.asarray(noise, np.float32)[:B, N_SLOTS:]
    robot = (int(first_robot) + np.arange(B, dtype=object)) % 2 ** 32
    g = variate(robot.astype(np.uint64)[:, None], int(step) % 2 ** 32, np.arange(N_SLOTS)[None, :], seed)
    n = bias.astype(np.float64) + sigma.astype(np.float64) * g.astype(np.float64)
    if s_std is not None:
        scale = np.ones(N_SLOTS)
        scale[s_first:] = np.asarray(s_std, np.float64)[s_first:]
        n = np.where(np.arange(N_SLOTS) >= s_first, n / scale, n)
    out = (X[:, :N_SLOTS].astype(np.float64) + n).astype(np.float32)
    touched = (sigma != 0) | (bias != 0)
    X[:, :N_SLOTS] = np.where(touched, out, X[:, :N_SLOTS])
    return X
