"""GPU checks of the push on nmpc_contact_track_batch: the pushed track is held bit for bit to the chain of pushed
nmpc_contact_step_batch calls with the window moved along (itself held to the fp64 reference in tests/test_gpu_push_step.py), and
detached it is the track it was.  The world is the standing world of tests/test_gpu_contact_track.py, built again here in small:
the tilted quadruped with feet at -3 mm / 0 / +2 cm, a small feed-forward torque, PD targets within 0.05 rad of STAND."""
import numpy as np
import pytest

from tests import contact_reference as cr
from tests import fd_reference as fr
from tests.torque_helpers import ground, layer, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KP, KD, DT = 20.0, 1.5, 5e-4
N_STEPS, N_SUB, FIRST, COUNT = 5, 3, 4, 7          # the window [4, 11) of 15 substeps: it starts inside step 1 and ends inside step 3
A_ROWS, QV_ROWS, SENTINEL = 7, 6, -77.0            # the tables are longer than the steps taken


class World:
    B = 33

    def __init__(self):
        self.m = m = fr.quadruped(perturb=0.3)
        self.L = layer(m)
        B = self.B
        q, v, tau, _ = fr.inputs(m, B, 258)
        lowest = lambda: np.array([cr.feet(m, q[b])[0][:, 2].min() for b in range(B)])      # noqa: E731
        want = np.array([-0.003, 0.0, 0.02])[np.arange(B) % 3]
        lift = (m.forward_kinematics(q[0])[0][2] @ m.axis[2])[2]
        q[:, 2] += ((want - lowest()) / lift).astype(np.float32)
        rng = np.random.default_rng(12)
        dev = lambda x: torch.as_tensor(np.asarray(x, np.float32), device=self.L.device)      # noqa: E731
        self.q, self.v, self.tau = dev(q), dev(v), dev(0.1 * tau)
        self.A = dev(fr.STAND[None, None, :] + rng.uniform(-0.05, 0.05, (B, A_ROWS, 12)))
        self.F = dev(rng.uniform(-80, 80, (B, 3)))

    def chain(self, B, pushed=True):
        """n_steps public contact steps, the window moved by n_sub per step -> (q, v, Q, V)"""
        L, q, v = self.L, self.q[:B], self.v[:B]
        Q, V = [], []
        for k in range(N_STEPS):
            Q.append(q); V.append(v)
            if pushed:
                L.set_push(self.F[:B], FIRST - N_SUB * k, COUNT)
            q, v = L.contact_step(q, v, DT, N_SUB, tau_ff=self.tau[:B], q_des=self.A[:B, k].contiguous(), kp=KP, kd=KD, ground=ground())[:2]
        L.set_push(None)
        return q, v, torch.stack(Q, 1), torch.stack(V, 1)

    def track(self, B, pushed=True, skip=None, skip_mask=0):
        L, q, v = self.L, self.q[:B].clone(), self.v[:B].clone()
        Qt, Vt = (torch.full((B, QV_ROWS, 18), SENTINEL, dtype=torch.float32, device=L.device) for _ in range(2))
        if pushed:
            L.set_push(self.F[:B], FIRST, COUNT)
        try:
            L.contact_track(q, v, self.A[:B, :N_STEPS], DT, N_SUB, tau_ff=self.tau[:B], kp=KP, kd=KD, ground=ground(), Q=Qt[:, :N_STEPS],
                            V=Vt[:, :N_STEPS], skip=skip, skip_mask=skip_mask)
        finally:
            L.set_push(None)
        return q, v, Qt[:, :N_STEPS], Vt[:, :N_STEPS], Qt, Vt


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.mark.parametrize("B", [1, 33])
def test_the_pushed_track_is_the_chain_of_pushed_steps_bit_for_bit(world, B):
    ref, got = world.chain(B), world.track(B)
    diff = [float((a - b).abs().max()) for a, b in zip(got[:4], ref)]
    print(f"B = {B}: largest |track - chain| of q, v, Q, V: {diff}")
    assert all(same(a, b) for a, b in zip(got[:4], ref))
    assert bool((got[4][:, N_STEPS:] == SENTINEL).all()) and bool((got[5][:, N_STEPS:] == SENTINEL).all())
    plain = world.chain(B, pushed=False)
    # rows 0 and 1 are written before the first pushed substep (4 = substep 1 of step 1), row 2 after it
    assert same(got[2][:, :2], plain[2][:, :2]) and same(got[3][:, :2], plain[3][:, :2])
    assert not same(got[3][:, 2], plain[3][:, 2]) and not same(got[1], plain[1])


@pytest.mark.parametrize("B", [1, 33])
def test_detached_the_track_is_the_unpushed_chain(world, B):
    ref = world.chain(B, pushed=False)
    assert all(same(a, b) for a, b in zip(world.track(B, pushed=False)[:4], ref))
    # and with a window that misses the call
    L = world.L
    for first, count in ((N_STEPS * N_SUB, 4), (-3, 3), (5, 0)):
        L.set_push(world.F[:B], first, count)
        try:
            q, v = world.q[:B].clone(), world.v[:B].clone()
            _, _, Q, V = L.contact_track(q, v, world.A[:B, :N_STEPS], DT, N_SUB, tau_ff=world.tau[:B], kp=KP, kd=KD, ground=ground())
        finally:
            L.set_push(None)
        assert all(same(a, b) for a, b in zip((q, v, Q, V), ref)), (first, count)


def test_skipped_robots_are_untouched_under_a_push(world):
    B = 33
    skip = torch.zeros(B, dtype=torch.int32, device=world.L.device)
    skip[::3] = 4 | 1
    skip[1::3] = 1
    q, v, Q, V, Qt, Vt = world.track(B, skip=skip, skip_mask=4)
    out, kept = torch.arange(B, device=q.device) % 3 == 0, torch.arange(B, device=q.device) % 3 != 0
    assert same(q[out], world.q[:B][out]) and same(v[out], world.v[:B][out])
    assert bool((Qt[out] == SENTINEL).all()) and bool((Vt[out] == SENTINEL).all())
    ref = world.chain(B)
    assert all(same(a[kept], b[kept]) for a, b in zip((q, v, Q, V), ref))
