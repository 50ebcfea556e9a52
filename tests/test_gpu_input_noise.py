"""GPU checks of input noise on training batches (nmpc_policy_set_input_noise, nmpc_policy_input_noise_epoch and
nmpc_policy_input_noise_batch behind `DevicePolicy.set_input_noise`, `input_noise_epoch`, `input_noise`; `train_epoch` while a vector
is attached; `learning.train_network(input_noise=...)`).

The rule is an exact integer, one fp32 product and a handful of fp64 operations that are each rounded once, and an attached epoch
runs the device code of the chain it fuses, so every comparison is equality of the bit patterns: the kernel against the numpy
restatement (tests/input_noise_reference.py), an attached epoch against idx -> db.batch -> input_noise -> train_step.

Shapes: a policy of 44 + 3 inputs, 12 outputs, two hidden layers of 32, with and without BatchNorm; a database of 64 rows, with and
without normalisation.  The noise kernel runs 256 threads per block over B x n (row, column) pairs: B = 6 with n = 44 is 264
pairs, a second block that starts inside row 5; epochs of 3 batches of 8 and of 5 rows, 5 being no multiple of the 4 rows a block
of the assembly kernel makes."""
import ctypes

import numpy as np
import pytest

from tests import input_noise_reference as ir
from tests.solve_helpers import dev  # noqa: F401
from tests.test_gpu_train_epoch import assert_same_optimizer_state, assert_same_state, same_bits
from tests.torque_helpers import same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_IN, N_OUT, LAYERS, HIDDEN, ROWS, LR = 47, 12, 2, 32, 64, 1e-3
SEED = 0x9E3779B97F4A7C15                                 # above 2^63: all 64 bits of the key are carried
SENTINEL = -77.0
_made = {}


def sigma_of(n):
    """n standard deviations in the units of the raw columns, columns 0 and 5 quiet"""
    s = np.random.default_rng(n).uniform(0.02, 0.3, n).astype(np.float32)
    s[[0, 5]] = 0.0
    return s


def database(norm):
    """64 rows with columns of distinct scales, made once per module and never changed by a test"""
    if norm not in _made:
        from iterative_learning_nmpc_amd.database import DeviceDatabase
        rng = np.random.default_rng(17)
        s = (rng.normal(0, 2, 44) + np.exp(rng.uniform(-2, 1, 44)) * rng.standard_normal((ROWS, 44))).astype(np.float32)
        s[:, 0] = np.round(rng.uniform(0, 1, ROWS), 4)
        db = DeviceDatabase(ROWS + 5, norm_input=norm)
        db.append(s, rng.standard_normal((ROWS, N_OUT)).astype(np.float32), vc_goals=rng.uniform(-0.5, 0.5, (ROWS, 3)).astype(np.float32))
        w = torch.tensor(np.where(rng.random(ROWS) < 0.2, 5.0, 1.0).astype(np.float32), device=db.device)
        _made[norm] = (db, w)
    return _made[norm]


def policy(bn, batch_max=8, seed=3):
    from iterative_learning_nmpc_amd.policy import DevicePolicy
    return DevicePolicy(N_IN, N_OUT, LAYERS, HIDDEN, bn, batch_max=batch_max, seed=seed)


def error_text(pol):
    return pol.lib.nmpc_policy_last_error(pol._h).decode()


def chain(pol, db, w, batch, n_batches, seed, epoch, lr=LR):
    """the chain the header states: the idx of the epoch, db.batch, input_noise at (epoch, t * batch), train_step"""
    from iterative_learning_nmpc_amd.policy import weighted_sample
    idx = weighted_sample(w, n_batches * batch, seed).reshape(n_batches, batch)
    s_std = db.states_std if db.norm_input else None
    losses = []
    for t in range(n_batches):
        x, y = db.batch(idx[t].contiguous())
        if epoch is not None:
            pol.input_noise(x, epoch, first_sample=t * batch, s_std=s_std, s_first=1)
        losses.append(pol.train_step(x, y, lr))
    return torch.cat(losses), idx


# ---- 1. the kernel against the restatement of its rule ------------------------------------------------------------------------------
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("x_stride", [47, 50])
@pytest.mark.parametrize("n", [44, 10])
def test_input_noise_is_the_reference(dev, n, x_stride, stats):
    pol = policy(False)
    B = 6
    rng = np.random.default_rng(100 * n + x_stride)
    X = rng.normal(0.0, 1.5, (B, x_stride)).astype(np.float32)
    X[:, n:] = SENTINEL
    X[:, [0, 5]] = SENTINEL
    sigma = sigma_of(n)
    s_std = rng.uniform(0.5, 2.0, 44) if stats else None
    pol.set_input_noise(sigma, seed=SEED, epoch0=11)
    # the plain case, a first sample that wraps past 2^32 inside the batch with an epoch above 2^16, and both counters past 2^32
    for epoch, first in ((0, 0), (2 ** 16 + 4465, 2 ** 32 - 3), (2 ** 32 + 7, 2 ** 33 + 2)):
        for s_first in (1, 0) if stats else (1,):
            got = pol.input_noise(torch.tensor(X, device=dev), epoch, first_sample=first, s_std=s_std, s_first=s_first)
            want = ir.input_noise(X, sigma, SEED, epoch, first, s_std, s_first)
            print(f"  n = {n}, x_stride = {x_stride}, stats = {stats}, s_first = {s_first}, epoch = {epoch}, first = {first}: largest "
                  f"|gpu - numpy| = {np.abs(got.cpu().numpy().astype(np.float64) - want).max():.3e}, moved {int((want != X).sum())} of {X.size}")
            assert same(got, torch.tensor(want, device=dev))
            assert bool((got[:, n:] == SENTINEL).all()) and bool((got[:, [0, 5]] == SENTINEL).all())      # from n on and the quiet columns
            assert int((want != X).sum()) == B * (n - 2)       # and everything else did move
            assert pol.input_noise_epoch == 11                 # the rule alone leaves the policy's epoch where it is
    # a slice of a wider tensor is taken with its stride, and another key draws other numbers
    wide = torch.tensor(np.concatenate([X, np.full((B, 4), SENTINEL, np.float32)], axis=1), device=dev)
    got = pol.input_noise(wide[:, :x_stride], 3, first_sample=8, s_std=s_std)
    assert same(got.contiguous(), torch.tensor(ir.input_noise(X, sigma, SEED, 3, 8, s_std), device=dev)) and bool((wide[:, x_stride:] == SENTINEL).all())
    pol.set_input_noise(sigma, seed=SEED + 1)
    other = pol.input_noise(torch.tensor(X, device=dev), 3, first_sample=8, s_std=s_std)
    assert not same(other[:, 1:5], got[:, 1:5])


# ---- 2. an attached epoch is the chain ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("batch", [8, 5])
def test_an_attached_epoch_is_the_chain_bit_for_bit(dev, batch, bn, norm):
    db, w = database(norm)
    fused, ref, clean = policy(bn), policy(bn), policy(bn)
    sigma, n_batches, seed = sigma_of(44), 3, 1234567891011
    fused.set_input_noise(sigma, seed=SEED, epoch0=70000)
    ref.set_input_noise(sigma, seed=SEED, epoch0=5)        # the chain names its epoch: the handle's own is not read
    losses, idx = fused.train_epoch(db, batch, n_batches, LR, seed, weights=w, return_idx=True)
    losses_ref, idx_ref = chain(ref, db, w, batch, n_batches, seed, 70000)
    assert same_bits(idx, idx_ref) and same_bits(losses, losses_ref), (losses, losses_ref)
    assert_same_state(fused, ref, "one attached epoch")
    assert_same_optimizer_state(fused, ref, "one attached epoch", n_batches)
    assert fused.input_noise_epoch == 70001 and ref.input_noise_epoch == 5
    # the second call draws at epoch0 + 1, a call without batches leaves the epoch
    assert fused.train_epoch(db, batch, 0, LR, seed, weights=w).shape == (0,) and fused.input_noise_epoch == 70001
    losses = fused.train_epoch(db, batch, n_batches, LR, seed + 1, weights=w)
    losses_ref, _ = chain(ref, db, w, batch, n_batches, seed + 1, 70001)
    assert same_bits(losses, losses_ref) and fused.input_noise_epoch == 70002
    assert_same_state(fused, ref, "two attached epochs")
    assert_same_optimizer_state(fused, ref, "two attached epochs", 2 * n_batches)
    # and the noise was not idle: the clean chain from the same parameters ends elsewhere
    chain(clean, db, w, batch, n_batches, seed, None)
    chain(clean, db, w, batch, n_batches, seed + 1, None)
    assert not same_bits(clean.get_parameters()[0], fused.get_parameters()[0])


@pytest.mark.parametrize("bn", [False, True])
def test_zero_sigma_and_a_detached_policy_give_the_bits_without(dev, bn):
    db, w = database(True)
    never, zeros, detached = policy(bn), policy(bn), policy(bn)
    zeros.set_input_noise(np.zeros(44, np.float32), seed=SEED)
    detached.set_input_noise(sigma_of(44), seed=SEED)
    detached.set_input_noise(None)
    assert detached.input_noise_epoch is None and detached._input_noise is None
    want = never.train_epoch(db, 5, 3, LR, 99, weights=w)
    for name, pol in (("zero sigma", zeros), ("detached", detached)):
        assert same_bits(pol.train_epoch(db, 5, 3, LR, 99, weights=w), want), name
        assert_same_state(pol, never, name)
        assert_same_optimizer_state(pol, never, name, 3)
    assert zeros.input_noise_epoch == 1                    # nothing is written, the epoch still counts


@pytest.mark.parametrize("bn", [False, True])
def test_loss_and_train_step_never_draw(dev, bn):
    db, _ = database(True)
    a, b = policy(bn, batch_max=16), policy(bn, batch_max=16)
    a.set_input_noise(sigma_of(44), seed=SEED, epoch0=4)
    x, y = db.batch(torch.arange(16, dtype=torch.int32, device=dev))
    keep = x.clone()
    assert same(a.loss(x, y), b.loss(x, y)) and same(a.forward(x), b.forward(x))
    assert same(a.train_step(x, y, LR), b.train_step(x, y, LR))
    assert_same_state(a, b, "train_step with a vector attached")
    assert_same_optimizer_state(a, b, "train_step with a vector attached", 1)
    assert same(x, keep) and a.input_noise_epoch == 4


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_attached_vector_in_force(dev):
    from iterative_learning_nmpc_amd._lib import NmpcError, ptr
    from iterative_learning_nmpc_amd.database import DeviceDatabase
    pol = policy(False)
    lib = pol.lib
    X = torch.full((6, N_IN), SENTINEL, device=dev)
    with pytest.raises(NmpcError, match="input noise: no table is attached"):
        pol.input_noise(X, 0)
    epoch = ctypes.c_longlong(-5)
    assert lib.nmpc_policy_input_noise_epoch(pol._h, ctypes.byref(epoch)) == -1 and "no table is attached" in error_text(pol) and epoch.value == -5
    sigma = sigma_of(44)
    pol.set_input_noise(sigma, seed=SEED, epoch0=21)
    assert lib.nmpc_policy_input_noise_epoch(pol._h, None) == -1 and "epoch is NULL" in error_text(pol)
    # n outside [1, n_in]: refused, and neither the vector nor its epoch is replaced
    other = torch.full((64,), 9.0, device=dev)
    for n in (0, -3, N_IN + 1):
        assert lib.nmpc_policy_set_input_noise(pol._h, ptr(other), n, 1, 2) == -1 and "1 <= n <= n_in" in error_text(pol)
    assert lib.nmpc_policy_set_input_noise(None, ptr(other), 44, 1, 2) == -1
    # what the rule alone does not take
    for args, text in (((6, None, N_IN, None, 1, 0, 0), "X is needed"), ((6, ptr(X), 43, None, 1, 0, 0), "x_stride must be at least n"),
                       ((6, ptr(X), N_IN, None, -1, 0, 0), "s_first must not be negative"), ((-1, ptr(X), N_IN, None, 1, 0, 0), "B >= 0")):
        assert lib.nmpc_policy_input_noise_batch(pol._h, *args, None) == -1 and text in error_text(pol), text
    assert lib.nmpc_policy_input_noise_batch(pol._h, 0, None, 0, None, 1, 0, 0, None) == 0      # an empty batch is no error
    with pytest.raises(ValueError, match="X: need at least the 44 columns"):
        pol.input_noise(X[:, :10].contiguous(), 0)
    # an epoch on a source with fewer state columns than the vector has entries: refused before any launch
    db, w = database(False)
    narrow = DeviceDatabase(16, n_state=40, n_vc_goal=7, norm_input=False)
    narrow.append(np.ones((8, 40), np.float32), np.ones((8, N_OUT), np.float32), vc_goals=np.ones((8, 7), np.float32))
    before = [t.clone() for t in pol.get_parameters()]
    with pytest.raises(NmpcError, match="input noise: n exceeds the n_state"):
        pol.train_epoch(narrow, 8, 1, LR, 1)
    torch.cuda.synchronize()
    assert bool((X == SENTINEL).all()) and all(same(a, b) for a, b in zip(before, pol.get_parameters())) and pol.get_optimizer_state()[2] == 0
    assert pol.input_noise_epoch == 21                     # nothing above drew or counted
    got = pol.input_noise(torch.zeros(6, N_IN, device=dev), 21)
    assert same(got, torch.tensor(ir.input_noise(np.zeros((6, N_IN), np.float32), sigma, SEED, 21), device=dev))      # the first vector and key


# ---- 4. through train_network ------------------------------------------------------------------------------------------------------------
def test_train_network_attaches_and_detaches_the_vector(dev):
    from iterative_learning_nmpc_amd import learning
    db, _ = database(True)
    sigma, n_epoch, batch = sigma_of(44), 2, 8
    n_batches = ROWS // batch
    val_idx = torch.arange(ROWS - 8, ROWS, dtype=torch.int32, device=dev)
    a, b, clean = policy(True), policy(True), policy(True)
    loss, val = learning.train_network(a, db, n_epoch, batch, lr=LR, seed=7, input_noise=sigma, input_noise_seed=SEED)
    assert a._input_noise is None and a.input_noise_epoch is None and loss.shape == (n_epoch, n_batches)
    # epoch e of the call draws at epoch e: the same epochs by hand
    b.set_input_noise(sigma, seed=SEED, epoch0=0)
    w = db.weights[:ROWS].clone()
    by_hand = torch.stack([b.train_epoch(db, batch, n_batches, LR, 7 + e, weights=w) for e in range(n_epoch)])
    assert same(loss, by_hand) and b.input_noise_epoch == n_epoch
    b.set_input_noise(None)
    assert_same_state(a, b, "train_network against its epochs")
    # validation is on clean rows: the loss of the rows as the database assembles them
    loss_v, val_v = learning.train_network(clean, db, 1, batch, lr=LR, seed=7, val_idx=val_idx, input_noise=sigma, input_noise_seed=SEED)
    assert same(val_v, clean.loss(*db.batch(val_idx))) and clean._input_noise is None
    assert not same(learning.train_network(policy(True), db, 1, batch, lr=LR, seed=7, val_idx=val_idx)[0], loss_v)      # the noise was not idle
    # detached also when the call raises, bad host input is refused on its way in, and a vector of the caller's is not replaced
    with pytest.raises(Exception):
        learning.train_network(a, db, 1, 0, input_noise=sigma)
    assert a._input_noise is None
    with pytest.raises(Exception):
        learning.train_network(a, db, 1, 64, input_noise=sigma)      # above batch_max: raised inside the epoch call
    assert a._input_noise is None and a.input_noise_epoch is None
    with pytest.raises(ValueError, match="input noise: sigma must not be negative"):
        learning.train_network(a, db, 1, batch, input_noise=-sigma - 1)
    assert a._input_noise is None
    a.set_input_noise(sigma, seed=5, epoch0=3)
    mine = a._input_noise
    with pytest.raises(ValueError, match="attached already"):
        learning.train_network(a, db, 1, batch, input_noise=sigma)
    assert a._input_noise is mine and a.input_noise_epoch == 3
    learning.train_network(a, db, 1, batch, lr=LR, seed=7)  # without the keyword the caller's vector stays, is used and counts
    assert a._input_noise is mine and a.input_noise_epoch == 4
