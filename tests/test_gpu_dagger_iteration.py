"""`learning.dagger_iteration`: the learner's rollout, the expert's labels for the states it visited, the rows that go into the
database, and the training on them.  B = 4 robots, T = 5 control steps, an untrained policy, one epoch of batches of 8."""
import pytest

from tests.plant_helpers import Dagger
from tests.solve_helpers import dev, policy_pair  # noqa: F401
from tests.torque_helpers import same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B, K, DT, N_SUB, T, SEED, BATCH = Dagger.B, Dagger.K, Dagger.DT, Dagger.N_SUB, Dagger.T, Dagger.SEED, Dagger.BATCH
setup = Dagger.setup


def run(w):
    from iterative_learning_nmpc_amd import learning
    out = learning.dagger_iteration(w["mpc"], w["layer"], w["db"], w["policy"], w["q0"], w["v0"], w["goal"], T, dt=DT, n_sub=N_SUB,
                                    n_epoch=1, batch_size=BATCH, lr=1e-3, seed=SEED, val_fraction=0.0)
    torch.cuda.synchronize()
    return out


def kept(out):
    """host copy of the selection the issue states: k < steps_survived[b] and a status that is neither NaN nor a QP failure"""
    from iterative_learning_nmpc_amd import _lib
    st, alive = out["status"].cpu().numpy(), out["steps_survived"].cpu().numpy()
    return [(b, k) for b in range(B) for k in range(K)
            if k < alive[b] and st[b, k] not in (_lib.NMPC_STATUS_NAN, _lib.NMPC_STATUS_QP)]


def test_rows_training_and_the_hand_filled_database(dev):
    from iterative_learning_nmpc_amd import learning
    from iterative_learning_nmpc_amd.database import DeviceDatabase
    w = setup(dev)
    out = run(w)
    idx = kept(out)
    print("steps survived", out["steps_survived"].tolist(), "statuses", out["status"].tolist(), "rows", out["n_rows"])
    assert out["Q"].shape == (B, K, 18) and out["A_star"].shape == (B, K, 12) and out["status"].shape == (B, K)
    assert out["n_rows"] == len(idx) == len(w["db"]) and len(idx) > 0
    bs, ks = (torch.as_tensor(x, device=dev) for x in zip(*idx))
    db = w["db"]
    assert same(db.tables["states"][:len(db)], out["S"][bs, ks]) and same(db.tables["actions"][:len(db)], out["A_star"][bs, ks])
    assert same(db.tables["vc_goals"][:len(db)], torch.as_tensor(w["goal"], device=dev)[bs])
    assert bool((db.weights[:len(db)] == 1.0).all())
    # the labels are the labeller's on the visited states, and the learner's actions are not the expert's
    A_ref, st_ref = w["mpc"].label_states(out["Q"], out["V"], w["layer"], dt_row=N_SUB * DT, failed=out["failed"])
    assert same(A_ref, out["A_star"]) and torch.equal(st_ref, out["status"])
    assert not same(out["A"], out["A_star"])
    # the same seed on a database filled by hand with those rows, from the same untrained parameters
    hand = DeviceDatabase(limit=256, norm_input=False, device=dev)
    hand.append(out["S"][bs, ks], out["A_star"][bs, ks], torch.as_tensor(w["goal"], device=dev)[bs])
    fresh = policy_pair(47, 12, 2, 64, False, 64, seed=3)[0]
    loss, _ = learning.train_network(fresh, hand, 1, BATCH, lr=1e-3, seed=SEED)
    assert out["train_loss"].shape == loss.shape == (1, -(-len(idx) // BATCH)) and same(out["train_loss"], loss)
    assert bool(torch.isnan(out["val_loss"]).all())


def test_a_robot_lying_on_the_ground_contributes_no_row(dev):
    w = setup(dev, lying=2)
    out = run(w)
    idx = kept(out)
    assert int(out["steps_survived"][2]) == 0 and not bool(out["survived"][2])
    assert all(b != 2 for b, _ in idx) and out["n_rows"] == len(idx) == len(w["db"]) > 0
    assert bool((out["A_star"][2] == 0).all()) and bool((out["status"][2] == 0).all())      # no solve was spent on it
