"""GPU checks of a ground per robot on the contact plant (nmpc_contact_set_grounds behind `BatchedTorqueLayer.set_grounds`).

Two kinds of claim.  Accuracy: with a table attached, robot b of `contact_forces`, `contact_step`, `contact_track` and the implicit
step is held to the fp64 reference (tests/contact_reference.py, tests/implicit_reference.py) run with that robot's `Ground`, under
`torque_helpers.bar`: max(1e-5 * scale, 4 x the deviation of the numpy-float32 run of the same reference loop from the fp64 run),
both computed here, never from the code under test.  Bits: robot b of a call with the table attached is robot b of the same call
-- same B, same row, same push -- with nothing attached and `ground = row b`; a table of equal rows is the uniform call; a policy
rollout is its chain of public calls; the expert on the plant is, rollout by rollout, the expert on the uniform plant of that row.
Those are `np.array_equal` / equality of the bit patterns.  Every figure is printed before it is asserted.

The fixture is the "tilted" quadruped case of tests/test_gpu_contact.py (fr.quadruped(perturb=0.3), fr.inputs(m, 257, 258), the
lowest foot at -3 mm / 0 / +2 cm in turn) at B = 33, one robot past a block, under 33 distinct rows."""
import ctypes

import numpy as np
import pytest

from tests import contact_reference as cr
from tests import fd_reference as fr
from tests import implicit_reference as ir
from tests import plant_helpers as ph
from tests.plant_helpers import AT, DT, DT_IMPLICIT, INTEGRATORS, KD, KP, N_SUB, NAMES, STEP_SUB, TRACK_NAMES
from tests.plant_helpers import World, default_policy, detached, expert, held_row_by_row, quadruped_layer, standing_start  # noqa: F401
from tests.solve_helpers import dev  # noqa: F401
from tests.torque_helpers import THREE_HEIGHTS, branches, held, host, layer, lower_feet, rows_equal, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B, SEED = 33, 7
K = ph.ROLLOUT_STEPS                                      # the track and the policy rollout: 3 control steps of N_SUB = 2 substeps
ROBOTS = (0, 31, 32)                                      # first lane, last lane of a block, the ragged tail


def device_ground(row):
    """the uniform `GroundContact` of one row of a table"""
    from iterative_learning_nmpc_amd.torque import GroundContact
    return GroundContact(*(float(x) for x in row[:5]), tau_max=float(row[5]) if row[5] > 0 else None)


def draw_rows(rng, n, ground_z, stiffness, damping, clamp):
    """n distinct rows: mu in [0.2, 1.2], slip_velocity in [0.02, 0.1], ground_z within 1 cm of the case's, stiffness and damping
    in the given ranges; tau_max 0 (no limit) for every third robot, in `clamp` for the next, ten times that for the last"""
    rows = np.zeros((n, 6), np.float32)
    rows[:, 0] = ground_z + rng.uniform(-0.01, 0.01, n)
    rows[:, 1] = rng.uniform(*stiffness, n)
    rows[:, 2] = rng.uniform(*damping, n)
    rows[:, 3] = rng.uniform(0.2, 1.2, n)
    rows[:, 4] = rng.uniform(0.02, 0.1, n)
    small = rng.uniform(*clamp, n)
    rows[:, 5] = np.where(np.arange(n) % 3 == 0, 0.0, np.where(np.arange(n) % 3 == 1, small, 10.0 * small))
    return rows


class Fixture(ph.Fixture):
    """The host side: states, inputs, the table and its references."""
    def __init__(self):
        self.m = m = fr.quadruped(perturb=0.3)
        q, v, tau, _ = fr.inputs(m, 257, 258)
        q, v, tau = lower_feet(m, q[:B], THREE_HEIGHTS[np.arange(B) % 3], tol=1e-6), v[:B].copy(), tau[:B].copy()
        self.q, self.v, self.tau = q.astype(np.float32), v.astype(np.float32), tau.astype(np.float32)
        self.q_des = (self.q[:, 6:] + np.random.default_rng(1).uniform(-0.1, 0.1, (B, 12))).astype(np.float32)
        rng = np.random.default_rng(SEED)
        self.rows = draw_rows(rng, B, 0.0, (5e3, 2e4), (1.0, 5.0), (2.0, 6.0))
        self.G = ph.grounds_of(self.rows)
        self.A = (self.q[:, None, 6:] + rng.uniform(-0.05, 0.05, (B, K, 12))).astype(np.float32)
        self.F = rng.uniform(-80, 80, (B, 3)).astype(np.float32)
        self.goal = rng.uniform(-0.5, 0.5, (B, 3)).astype(np.float32)
        k64 = [cr.feet(m, self.q[b], self.v[b]) for b in range(B)]
        k32 = [cr.feet(m, self.q[b], self.v[b], np.float32) for b in range(B)]
        self.pos, self.vel = np.stack([k[0] for k in k64]), np.stack([k[1] for k in k64])
        self.f = np.stack([cr.contact_law(self.G[b], self.pos[b], self.vel[b]) for b in range(B)])
        self.f32 = np.stack([cr.contact_law(self.G[b], k32[b][0], k32[b][1]) for b in range(B)])
        assert self.f32.dtype == np.float32
        self.freeze()

    def step(self, n_sub):
        """(fp64, float32) outputs of contact_step_ref per robot under its own Ground, stacked"""
        run = lambda **kw: [np.stack(x) for x in zip(*[cr.contact_step_ref(self.m, self.G[b], self.q[b], self.v[b], DT, n_sub, self.tau[b],  # noqa: E731
                                                                               self.q_des[b], KP, KD, **kw) for b in range(B)])]
        return self.cached(n_sub, lambda: (run(), run(fd=fr.aba, dtype=np.float32)))

    def track(self, **kw):
        """the chained reference: K control steps of N_SUB substeps with q_des = A[b, k] -> (q, v, Q, V) stacked over the robots"""
        out = []
        for b in range(B):
            q, v, Q, V = self.q[b], self.v[b], [], []
            for k in range(K):
                Q.append(np.array(q)); V.append(np.array(v))
                q, v = cr.contact_step_ref(self.m, self.G[b], q, v, DT, N_SUB, self.tau[b], self.A[b, k], KP, KD, **kw)[:2]
            out.append((q, v, np.stack(Q), np.stack(V)))
        return [np.stack(x) for x in zip(*out)]

    def implicit(self, n_sub, dtype):
        return [np.stack(x) for x in zip(*[ir.implicit_step_ref(self.m, self.G[b], self.q[b], self.v[b], DT_IMPLICIT, n_sub, self.tau[b], self.q_des[b],
                                                               KP, KD, dtype=dtype) for b in range(B)])]

    def conditions(self):
        """what the issue asks of the fixture, from the fp64 reference alone"""
        ref = self.step(1)[0]
        off = pushed = leaving = 0
        for b in range(B):
            o, p, l = branches(self.G[b], self.pos[b], self.vel[b], self.f[b])
            off, pushed, leaving = off + o, pushed + p, leaving + l
        limits = np.array([np.inf if g.tau_max is None else g.tau_max for g in self.G])
        clamped = np.abs(ref[4]) == limits[:, None]
        print(f"fixture: feet off the ground {off}, pushed {pushed}, leaving too fast to be pushed {leaving}; torques clamped {int(clamped.sum())} of "
              f"{clamped.size}, robots with no torque clamped {int((~clamped.any(axis=1)).sum())}")
        assert off and pushed and leaving
        assert clamped.any() and (~clamped.any(axis=1)).any()
        assert np.all(self.rows[0] != self.rows[1])                                   # two robots of one wave differ in every column
        assert len({tuple(r) for r in self.rows.tolist()}) == B                        # 33 distinct rows
        at = np.abs(self.rows[:, 0, None].astype(np.float64) - self.pos[..., 2]) < AT
        assert not at.any()              # no foot at its own plane: the implicit scheme has one reference per robot (test_gpu_contact_implicit.py)


@pytest.fixture(scope="module")
def fx():
    f = Fixture()
    f.conditions()                       # asserted before anything else
    return f


@pytest.fixture(scope="module")
def world(fx):
    return World(fx.m, B, q=fx.q, v=fx.v, tau=fx.tau, q_des=fx.q_des, A=fx.A, F=fx.F, goal=fx.goal)


# ---- 1. forces, step, track and the implicit step against the reference -----------------------------------------------------------------
def test_forces_match_the_law_of_each_robots_row(fx, world, detached):
    world.L.set_grounds(fx.rows)
    f, = host(*world.forces())
    print("forces under the table, B 33")
    assert f.shape == (B, 4, 3) and held("f", f, fx.f, fx.f32)
    assert np.all(f[..., 2] >= 0)


@pytest.mark.parametrize("n_sub", [1, STEP_SUB])
def test_the_step_matches_the_reference_of_each_robots_row(fx, world, detached, n_sub):
    ref, f32 = fx.step(n_sub)
    world.L.set_grounds(fx.rows)
    got = host(*world.step(n_sub=n_sub))
    assert [x.shape for x in got] == [(B, 18)] * 3 + [(B, 4, 3), (B, 12)]
    print(f"step under the table, {n_sub} substeps, B 33")
    assert all([held(name, x, r, f) for name, x, r, f in zip(NAMES, got, ref, f32)])


def test_the_track_matches_the_chained_reference(fx, world, detached):
    ref, f32 = fx.track(), fx.track(fd=fr.aba, dtype=np.float32)
    world.L.set_grounds(fx.rows)
    got = host(*world.track())
    assert [x.shape for x in got] == [(B, 18)] * 2 + [(B, K, 18)] * 2
    print(f"track under the table, {K} control steps of {N_SUB} substeps, B 33")
    assert all([held(name, x, r, f) for name, x, r, f in zip(TRACK_NAMES, got, ref, f32)])


@pytest.mark.parametrize("n_sub", [1, STEP_SUB])
def test_the_implicit_step_matches_the_reference_of_each_robots_row(fx, world, detached, n_sub):
    ref, f32 = fx.implicit(n_sub, np.float64), fx.implicit(n_sub, np.float32)
    world.L.set_integrator("implicit")
    world.L.set_grounds(fx.rows)
    got = host(*world.step(n_sub=n_sub, dt=DT_IMPLICIT))
    print(f"implicit step under the table, {n_sub} substeps of {DT_IMPLICIT} s, B 33")
    assert all([held(name, x, r, f) for name, x, r, f in zip(NAMES, got, ref, f32)])


# ---- 2. robot b is the bits of the uniform call under its own row ----------------------------------------------------------------------
FIRST = [1 + 2 * (b % 2) for b in range(B)]               # windows per robot: every one starts inside a control step of the track (odd
COUNT = [1 + b % 3 for b in range(B)]                     # substeps of N_SUB = 2) and inside the step's four substeps
PUSHES = {"none": None, "one window": {"step": (1, 2), "track": (3, 2)}, "windows": {"step": (FIRST, COUNT), "track": (FIRST, COUNT)}}


@pytest.mark.parametrize("push", list(PUSHES))
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_robot_b_is_the_uniform_call_under_its_row(fx, world, detached, integrator, push):
    L = world.L
    L.set_integrator(integrator)
    calls = {"step": (world.step, NAMES), "track": (world.track, TRACK_NAMES)}
    if push == "none":
        calls["forces"] = (world.forces, ("f",))

    def uniform_of(b):                                      # nothing attached, and the ground of the call is row b
        L.set_grounds(None)
        return dict(g=device_ground(fx.rows[b]))
    for name, (call, outputs) in calls.items():
        if PUSHES[push] is not None:
            L.set_push(world.F, *PUSHES[push][name])
            assert (L._push_windows is not None) == (push == "windows")
        plain = call()
        got, _ = held_row_by_row(call, lambda: L.set_grounds(fx.rows), uniform_of, ROBOTS, outputs,
                                 lambda b, o: f"{integrator}, push {push}, {name}, robot {b} {o}: largest |table - uniform|")      # noqa: B023
        assert not all(rows_equal(got, plain, b) for b in ROBOTS), name      # and the rows matter: the default ground gives other bits
        L.set_push(None)


# ---- 3. a table of equal rows is the uniform call ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_a_table_of_equal_rows_is_the_uniform_call(world, detached, integrator):
    from iterative_learning_nmpc_amd.torque import GroundContact
    L = world.L
    L.set_integrator(integrator)
    plain = world.step() + world.track() + world.forces()
    L.set_grounds([GroundContact()] * B)
    got = world.step() + world.track() + world.forces()
    assert all(same(x, y) for x, y in zip(got, plain))
    L.set_grounds(None)
    assert L._grounds is None
    again = world.step() + world.track() + world.forces()
    assert all(same(x, y) for x, y in zip(again, plain))


# ---- 4. a block width that changes -------------------------------------------------------------------------------------------------------
SOFT = dict(stiffness=(100.0, 300.0), damping=(0.2, 0.8))  # tests/test_gpu_contact.py: these feet lie up to a metre in the ground
GENERAL = {"tree23": (lambda: fr.random_tree(), 96, 5), "tree30": (lambda: fr.random_tree(n=30, seed=13, feet=(4, 29, 29, 17)), 40, 6)}


@pytest.mark.parametrize("tree", list(GENERAL))
def test_general_trees_step_under_a_table(tree):
    """tree23 (23 joints, B = 96) is the widest tree of the 32-robot block, tree30 (B = 40) runs the 16-robot block: the trees on the
    two sides of the boundary that the law per lane moves by 24 bytes a robot."""
    make, n_robots, seed = GENERAL[tree]
    m = make()
    q, v, tau, _ = fr.inputs(m, n_robots, seed)
    z = float(np.float32(np.median([cr.feet(m, q[b])[0][:, 2] for b in range(n_robots)])))
    q_des = (q[:, m.n - m.nu:] + np.random.default_rng(3).uniform(-0.1, 0.1, (n_robots, m.nu))).astype(np.float32)
    rows = draw_rows(np.random.default_rng(SEED), n_robots, z, SOFT["stiffness"], SOFT["damping"], (2.0, 6.0))
    G = ph.grounds_of(rows)
    run = lambda **kw: [np.stack(x) for x in zip(*[cr.contact_step_ref(m, G[b], q[b], v[b], DT, 1, tau[b], q_des[b], KP, KD, **kw)  # noqa: E731
                                                   for b in range(n_robots)])]
    ref, f32 = run(), run(fd=fr.aba, dtype=np.float32)
    inside = rows[:, 0, None] - np.stack([cr.feet(m, q[b])[0][:, 2] for b in range(n_robots)]) > 0
    print(f"{tree}: feet in the ground {int(inside.sum())} of {inside.size}")
    assert inside.any() and (~inside).any()
    L = layer(m)
    L.set_grounds(rows)
    got = host(*L.contact_step(q, v, DT, 1, tau_ff=tau, q_des=q_des, kp=KP, kd=KD))
    print(f"{tree}: one substep under the table, B {n_robots}")
    assert all([held(name, x, r, f) for name, x, r, f in zip(NAMES, got, ref, f32)])


# ---- 5. policy in the loop ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def policy(world):
    return default_policy()


def test_the_policy_rollout_is_its_chain_of_public_calls(fx, world, policy, detached):
    ph.policy_rollout_is_its_chain_of_public_calls(world, policy, "grounds", fx.rows)


def test_evaluate_policy_attaches_and_detaches_the_table(fx, world, policy, detached):
    ph.evaluate_policy_attaches_and_detaches_the_table(world, policy, "grounds", fx.rows)


# ---- 6. the expert on the plant ----------------------------------------------------------------------------------------------------------
def test_the_expert_on_the_plant_stands_on_each_rollouts_row(dev, quadruped_layer):
    """B = 3 rollouts, 2 replans (T = 0.0795 s, tests/test_gpu_wb_plant_rollout.py), three different rows: rollout b against
    rollout b of the same call with nothing attached and plant = GroundContact(row b)."""
    from iterative_learning_nmpc_amd.torque import GroundContact
    L = quadruped_layer
    rows = np.array([[0.0, 1e4, 3.0, 0.8, 0.05, 0.0], [0.004, 1.5e4, 2.0, 0.5, 0.04, 30.0], [-0.003, 8e3, 4.0, 1.1, 0.08, 18.0]], np.float32)
    q0, v0 = standing_start(3)

    def run(plant):
        mpc = expert(dev, 3)
        S = mpc.open_loop_device(q0, v0, 0.0795, torque_layer=L, plant=plant, plant_substeps=2)
        return S, mpc.actions, mpc.q_final, mpc.v_final, mpc.failed

    L.set_grounds(rows)
    got = run(GroundContact())
    L.set_grounds(None)
    assert got[0].shape == (3, 80, 44) and bool(torch.isfinite(got[0]).all())
    refs = [run(device_ground(rows[b])) for b in range(3)]
    for b in range(3):
        for name, x, y in zip(("S", "A", "q", "v"), got, refs[b]):
            print(f"  rollout {b} {name}: largest |table - uniform| {float((x[b].double() - y[b].double()).abs().max()):.3e}")
    for b in range(3):
        assert all(same(x[b], y[b]) for x, y in zip(got[:4], refs[b][:4])) and int(got[4][b]) == int(refs[b][4][b]), b
    assert not same(got[0][1], refs[0][0][1])                                          # and the rows matter


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_detaching_and_the_empty_batch(fx, world, detached):
    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd._lib import NmpcError
    from iterative_learning_nmpc_amd.torque import GroundContact
    L, lib = world.L, world.L.lib
    text = lambda: lib.nmpc_torque_last_error(L._h).decode()                           # noqa: E731
    table = torch.as_tensor(fx.rows[:4].copy(), device=L.device)
    # B > n_rows, in every call that honours the table
    L.set_grounds(table)
    assert L._grounds is table                                                         # a device tensor is taken as given
    for call in (world.step, world.track, world.forces):
        with pytest.raises(NmpcError, match="grounds: B exceeds n_rows"):
            call()
    with pytest.raises(NmpcError, match="grounds: B exceeds n_rows"):
        L.policy_rollout(default_policy(), world.q, world.v, 1, DT, 1, world.goal)
    assert [tuple(x.shape) for x in L.contact_step(world.q[:4], world.v[:4], DT, 1)] == [(4, 18)] * 3 + [(4, 4, 3), (4, 12)]
    # cfg is still validated under a table
    with pytest.raises(NmpcError, match="slip_velocity must be positive"):
        L.contact_step(world.q[:4], world.v[:4], DT, 1, ground=GroundContact(slip_velocity=0.0))
    # the empty batch
    st, cfg = _lib.stream(L.device), ctypes.byref(GroundContact().cfg())
    assert lib.nmpc_contact_step_batch(L._h, 0, 1, DT, cfg, None, None, None, None, KP, KD, None, None, None, None, None, st) == 0
    assert lib.nmpc_contact_forces_batch(L._h, 0, cfg, None, None, None, st) == 0
    # n_rows < 1 with a table: refused, what was attached stays
    assert lib.nmpc_contact_set_grounds(L._h, _lib.ptr(table), 0) == -1 and "n_rows must be at least 1" in text()
    with pytest.raises(NmpcError, match="grounds: B exceeds n_rows"):
        world.step()
    # a NULL handle
    assert lib.nmpc_contact_set_grounds(None, _lib.ptr(table), 4) == -1
    assert b"handle" in lib.nmpc_torque_last_error(None)
    # detaching twice is fine
    assert lib.nmpc_contact_set_grounds(L._h, None, 0) == 0 and lib.nmpc_contact_set_grounds(L._h, None, 0) == 0
    L.set_grounds(None); L.set_grounds(None)
    assert [tuple(x.shape) for x in world.step()] == [(B, 18)] * 3 + [(B, 4, 3), (B, 12)]
    # the layer's own checks of a device table
    with pytest.raises(ValueError, match="device table"):
        L.set_grounds(torch.zeros(4, 5, device=L.device))
