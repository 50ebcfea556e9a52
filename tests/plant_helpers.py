"""What the contact-plant tests and the rollouts on the plant share (helper module, not collected by pytest): the plant's constants,
the host `Fixture` base, the draws and worlds that more than one file uses, the device `World`, `detach` with its fixture, the
row-by-row comparison of a call under a table per robot with the same call under one row for all, the set-up of the whole-body
expert on the plant, and the scenarios that hold for every table per robot up to its name, its rows and how it is attached.  A test
file keeps its references, its case tables and what is particular to its table; a shared scenario is called from a test of the
file's own, which keeps its name and parametrisation.

Fixtures are shared by import:  from tests.plant_helpers import detached, quadruped_layer  # noqa: F401"""
import numpy as np
import pytest

from tests.torque_helpers import layer, rows_equal

# ---- the plant as the tests drive it; a file that uses another value states its own and says so ----------------------------------------
KP, KD, DT, DT_IMPLICIT = 20.0, 1.5, 5e-4, 1e-3
N_SUB, STEP_SUB = 2, 4                                    # substeps per control step of a track or a policy rollout, of a single step
ROLLOUT_STEPS = 3                                         # control steps of a policy rollout
PERIOD, T0, HEIGHT, MASK = 0.5, 0.37, 0.08, 2 | 4 | 8 | 32
INTEGRATORS = ("explicit", "implicit")
NAMES, TRACK_NAMES = ("q", "v", "a", "f", "tau"), ("q", "v", "Q", "V")
AT = 1e-6                                                 # a foot this close to its plane is "at" it (tests/test_gpu_contact_implicit.py)


def default_policy():
    """the policy of the plant's policy rollouts: 44 + 3 inputs, one hidden layer of 64 with batch norm, non-trivial parameters"""
    from tests.solve_helpers import policy_pair
    return policy_pair(47, 12, 1, 64, True, 64, seed=5)[0]


def device_policy(oracle, batch_max):
    """the DevicePolicy with the parameters of a policy oracle"""
    from iterative_learning_nmpc_amd.policy import DevicePolicy
    n_in, n_out, L, hidden, bn = oracle.dims
    p = DevicePolicy(n_in, n_out, L, hidden, bn, batch_max=batch_max, seed=None)
    p.set_parameters(oracle.theta.astype(np.float32), oracle.running_mean.astype(np.float32), oracle.running_var.astype(np.float32))
    return p


# ---- the host side ------------------------------------------------------------------------------------------------------------------------
class Fixture:
    """The host side of a plant test: arrays that are built once and never written to, and references computed once per key.  No
    device is touched, so the conditions on a fixture can be checked on a machine without one.  A subclass draws its arrays in
    `__init__`, ends it with `freeze()`, and states its own references and `conditions()`."""
    def freeze(self):
        self._refs = {}
        for x in vars(self).values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)

    def cached(self, key, make):
        if key not in self._refs:
            self._refs[key] = make()
        return self._refs[key]


TRUNK = 5                                                 # the body a payload hangs on and a push acts on
ACTUATOR_UPPER = (1.5 * KP, 1.5 * KD, 0.2, 0.02)


def draw_payloads(rng, n):
    """n rows: m_p in [0, 5] kg -- robot 0 carries nothing, robot 1 the full 5 kg --, r uniform in direction with |r| <= 0.15 m"""
    rows = np.zeros((n, 4), np.float32)
    rows[:, 0] = rng.uniform(0.0, 5.0, n)
    rows[0, 0] = 0.0
    if n > 1:
        rows[1, 0] = 5.0
    r = rng.standard_normal((n, 3))
    rows[:, 1:] = r / np.linalg.norm(r, axis=1, keepdims=True) * rng.uniform(0.0, 0.149, (n, 1))
    assert np.linalg.norm(rows[:, 1:].astype(np.float64), axis=1).max() <= 0.15
    return rows


def draw_actuators(rng, n):
    """n distinct rows: kp in KP x [0.5, 1.5], kd in KD x [0.5, 1.5], damping in [0, 0.2] N m s/rad, armature in [0, 0.02] kg m^2; the
    first four are the named ones: nominal, all four at their upper ends, armature only, damping only"""
    rows = np.stack([rng.uniform(0.5 * KP, 1.5 * KP, n), rng.uniform(0.5 * KD, 1.5 * KD, n), rng.uniform(0.0, 0.2, n), rng.uniform(0.0, 0.02, n)], axis=1)
    named = [(KP, KD, 0.0, 0.0), ACTUATOR_UPPER, (KP, KD, 0.0, 0.013), (KP, KD, 0.11, 0.0)]
    rows[:min(n, 4)] = named[:n]
    return rows.astype(np.float32)


def grounds_of(rows):
    """the reference `Ground` of every row of a float32 table of grounds (tau_max 0: no limit), from the float32 values themselves"""
    from tests import contact_reference as cr
    return [cr.Ground(*(float(x) for x in r[:5]), tau_max=float(r[5]) if r[5] > 0 else None) for r in rows]


def start_states(m, n, rng, slide=2):
    """the standing pose with +-0.1 rad on every joint and +-0.05 on the base attitude, velocities within +-1, and joint `slide`
    (the vertical base slider) set so that the lowest foot is at +2 cm ... -2 cm over the robots"""
    from tests import fd_reference as fr
    from tests.torque_helpers import lower_feet
    q = np.zeros((n, m.n)); q[:, 3:6] = rng.uniform(-0.05, 0.05, (n, 3)); q[:, 6:] = fr.STAND + rng.uniform(-0.1, 0.1, (n, 12))
    q[:, :2] = rng.uniform(-0.2, 0.2, (n, 2)); q[:, slide] = 0.3
    v = rng.uniform(-1.0, 1.0, (n, m.n))
    # Above the ground from 2 cm down to 1 mm, inside it from 4 mm to 2 cm, and nobody in between: a foot z of 0.3 m of kinematics
    # carries an error of a float32 ulp or two (2^-25 m), which the law turns into k x that = 3e-4 N of force whatever the depth,
    # while the bar's floor for a robot that touches at depth d is 1e-5 k d: below d = 3 mm the floor is under what the number
    # format owes and the bar would rest on the luck of the one float32 run that is its other term.
    want = np.concatenate([np.linspace(0.02, 0.001, n // 2), np.linspace(-0.004, -0.02, n - n // 2)]) if n > 1 else np.array([-0.01])
    # float32 before the correction, and a second pass that takes out what float32 left of the first
    return lower_feet(m, q, want, slide, passes=2, dtype=np.float32), v.astype(np.float32)


def tree32():
    """a 32-joint tree for the 16-wide blocks: the quadruped with 14 more one-joint bodies (a tail and a neck of revolute and
    prismatic joints in turn) hanging on its trunk, all behind the legs in joint order so the base and the feet stay where they are"""
    from oracle import torque_oracle as to
    from tests import fd_reference as fr
    m = fr.quadruped()
    rng = np.random.default_rng(23)
    extra = 32 - m.n
    parent = list(m.parent) + [TRUNK if i % 7 == 0 else m.n + i - 1 for i in range(extra)]
    jtype = list(m.jtype) + [i % 2 for i in range(extra)]
    axis = rng.standard_normal((extra, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    inertia = np.tile([2e-4, 0, 0, 2e-4, 0, 2e-4], (extra, 1))
    return to.TreeModel(parent, jtype, np.vstack([m.axis, axis]), np.concatenate([m.R_fix, np.tile(np.eye(3), (extra, 1, 1))]),
                        np.vstack([m.p_fix, 0.05 * rng.standard_normal((extra, 3))]), np.concatenate([m.mass, rng.uniform(0.05, 0.2, extra)]),
                        np.vstack([m.com, 0.02 * rng.standard_normal((extra, 3))]), np.vstack([m.inertia, inertia]), m.foot_joint, m.foot_offset,
                        n_actuated=12 + extra, gravity=m.gravity)


def wide_world(K=5):
    """B = 17 on the 32-joint tree, K control steps: the first 18 coordinates are the quadruped's start states, the appended joints
    start in +-0.3"""
    from tests import fd_reference as fr
    m = tree32()
    rng = np.random.default_rng(29)
    n, extra = 17, m.n - 18
    q18, v18 = start_states(fr.quadruped(), n, rng)
    q = np.hstack([q18, rng.uniform(-0.3, 0.3, (n, extra)).astype(np.float32)])
    v = np.hstack([v18, rng.uniform(-1, 1, (n, extra)).astype(np.float32)])
    tau = rng.uniform(-2, 2, (n, m.nu)).astype(np.float32)
    q_des = (q[:, 6:] + rng.uniform(-0.1, 0.1, (n, m.nu))).astype(np.float32)
    A = (q[:, None, 6:] + rng.uniform(-0.05, 0.05, (n, K, m.nu))).astype(np.float32)
    return World(m, n, q=q, v=v, tau=tau, q_des=q_des, A=A)


# ---- the device side ----------------------------------------------------------------------------------------------------------------------
class World:
    """The device side: one layer (of oracle tree `tree`, or `tree` itself where it is a layer already), the first n robots of the
    host `arrays` (q, v and whichever of tau, q_des, A, F, goal the file has) as tensors, the ground that every call passes
    (None: the default one) and the substeps of a control step and of a single step."""
    def __init__(self, tree, n, ground=None, n_sub=N_SUB, step_sub=STEP_SUB, **arrays):
        import torch
        from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
        self.L = tree if isinstance(tree, BatchedTorqueLayer) else layer(tree)
        self.n, self.ground, self.n_sub, self.step_sub = n, ground, n_sub, step_sub
        self.d = lambda x: torch.as_tensor(np.array(x), device=self.L.device).contiguous()      # noqa: E731
        self.tau = self.q_des = None
        self.arrays = tuple(arrays)
        for name, x in arrays.items():
            setattr(self, name, self.d(x[:n]))
        self.record = self.L.n == 18 and self.L.nu == 12    # the rows Q, V need the whole-body tree

    def permuted(self, perm):
        """the world of the robots `perm` (a permutation, or a selection such as the first four) on the same layer"""
        import torch
        w = World.__new__(World)
        w.__dict__.update(self.__dict__)
        p = torch.as_tensor(perm, device=self.L.device)
        w.n = len(perm)
        for name in self.arrays:
            setattr(w, name, getattr(self, name)[p].contiguous())
        return w

    def _ground(self, g):
        from iterative_learning_nmpc_amd.torque import GroundContact
        return g or self.ground or GroundContact()

    def step(self, n_sub=None, dt=DT, g=None):
        return self.L.contact_step(self.q, self.v, dt, n_sub or self.step_sub, tau_ff=self.tau, q_des=self.q_des, kp=KP, kd=KD, ground=self._ground(g))

    def track(self, dt=DT, g=None, **kw):
        out = self.L.contact_track(self.q.clone(), self.v.clone(), self.A, dt, self.n_sub, tau_ff=self.tau, kp=KP, kd=KD, ground=self._ground(g),
                                   record=self.record, **kw)
        return out if self.record else out[:2]

    def forces(self, g=None):
        return (self.L.contact_forces(self.q, self.v, self._ground(g)),)

    def rollout(self, policy, dt=DT):
        return self.L.policy_rollout(policy, self.q, self.v, ROLLOUT_STEPS, dt, self.n_sub, self.goal, tau_ff=self.tau, kp=KP, kd=KD,
                                     ground=self._ground(None), t0=T0, period=PERIOD, terminate_mask=MASK, collision_height=HEIGHT)


def detach(L):
    """everything a layer can hold, undone in one fixed order; what is not attached costs a library call at the most"""
    from iterative_learning_nmpc_amd.torque import TABLES
    for name in TABLES:
        getattr(L, "set_" + name)(None)
    L.set_push(None)                                      # with its windows
    L.set_rollout_states(None)
    L.set_rollout_observed(None)
    L.set_integrator("explicit")


def error_text(L):
    """the last error of the layer's handle as the library words it"""
    return L.lib.nmpc_torque_last_error(L._h).decode()


@pytest.fixture()
def detached(request):
    """whatever a test attaches or sets is gone after it, also when it fails: on the layer of the module's `world`, or, where the
    module has a world per tree (its `runs`), on the layer of every world made so far"""
    holder = request.getfixturevalue("world" if "world" in request.fixturenames else "runs")
    yield
    for L in [holder.L] if hasattr(holder, "L") else [r.c.L for r in holder.values()]:
        detach(L)


def held_row_by_row(call, attach_table, attach_uniform_of, robots, names, label, plain=None, moved_by=None):
    """`call()` with the table per robot attached (`attach_table()`) against `call()` under the uniform setting of robot b's row
    (`attach_uniform_of(b)`, which may return keywords for that call), for every b of `robots`: the largest difference of each
    output is printed as `label(b, name)`, then row b of the two is held bit for bit.  `call` returns a tuple in the order of
    `names`, or a dict with `names` among its keys.  -> (got, moved): the outputs under the table, and per chosen robot whether
    its uniform call differs from `plain` (the outputs with nothing attached) in the outputs `moved_by` (None: every one)."""
    attach_table()
    got = call()
    keys = names if isinstance(got, dict) else None
    moved = []
    for b in robots:
        ref = call(**(attach_uniform_of(b) or {}))
        for i, name in enumerate(names):
            x, y = (got[name], ref[name]) if keys else (got[i], ref[i])
            print(f"  {label(b, name)} {float((x[b].double() - y[b].double()).abs().max()):.3e}")
        assert rows_equal(got, ref, b, keys), b
        moved.append(plain is not None and not rows_equal(ref, plain, b, moved_by if keys else None))
    return got, moved


# ---- the whole-body expert on the plant ---------------------------------------------------------------------------------------------------
STEPS = 40                                                # simulation steps of 1 ms per replan, N_SUB substeps each on the plant
ONE, TWO, THREE, FIVE = 0.0395, 0.0795, 0.1195, 0.1995   # T of open_loop_device whose float clock runs exactly 1, 2, 3, 5 replans
SOLVER, SHIFT = 1, 8                                      # the solver bit of `failed`, and where the stamp of the replan starts


@pytest.fixture(scope="module")
def quadruped_layer(dev):
    from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
    from iterative_learning_nmpc_amd.workloads import quadruped_tree
    return BatchedTorqueLayer(**quadruped_tree(), device=dev)


def expert(dev, B=3, **kw):
    """the controller that lets the robot stand: the soft stance penalty around each leg's share of the weight"""
    from iterative_learning_nmpc_amd.mpc_wholebody import LocomotionMPC
    return LocomotionMPC(print_info=False, device=dev, batch=B, force_reference="gravity_share", **kw)


def standing_start(B=3):
    """(q0, v0) [B, 18] in float64: the base 0.30 m up, the joints at Q_HOME, at rest"""
    from iterative_learning_nmpc_amd import wholebody as wbk
    q0 = np.zeros((B, 18)); q0[:, 2] = 0.30; q0[:, 6:] = wbk.Q_HOME
    return q0, np.zeros((B, 18))


def default_plant():
    from iterative_learning_nmpc_amd.torque import GroundContact
    return GroundContact()


def plant_rollout(mpc, L, q0, v0, T=None, sync=False, plans=True, **kw):
    """one plant-mode `open_loop_device` on the default plant at N_SUB substeps -> what it leaves, by name; sync: wait for the
    device before reading; plans: with copies of the last plans X, U, the tracked reference and the solver status"""
    import torch
    S = mpc.open_loop_device(q0, v0, T, torque_layer=L, plant=default_plant(), plant_substeps=N_SUB, **kw)
    if sync:
        torch.cuda.synchronize()
    out = dict(S=S, A=mpc.actions, q=mpc.q_final, v=mpc.v_final, failed=mpc.failed)
    if plans:
        out.update(X=mpc._X_dev.clone(), U=mpc._U_dev.clone(), ref=np.array(mpc.base_ref_vel_tracking), status=mpc.status_dev)
    return out


def chain_of_public_calls(mpc, L, X, U, q0, v0, status, replan=0, mask=None):
    """labels -> track -> observe of one replan through the Python layer, then the harness' bookkeeping -> S, A, q, v, failed"""
    import torch
    from iterative_learning_nmpc_amd.config import COLLISION_HEIGHT, TERMINATE_DEFAULT
    mask = TERMINATE_DEFAULT if mask is None else mask
    d = L.device
    zoh = mpc.id_repeat[:STEPS]
    A = L.plan_actions(X, U, zoh, mpc.config_opt.time_horizon / mpc.config_opt.n_nodes, mpc.sim_dt, kp=mpc.Kp, kd=mpc.Kd)
    q = torch.as_tensor(np.array(q0), dtype=torch.float32, device=d).contiguous()
    v = torch.as_tensor(np.array(v0), dtype=torch.float32, device=d).contiguous()
    q, v, Q, V = L.contact_track(q, v, A, mpc.sim_dt / N_SUB, N_SUB, kp=mpc.Kp, kd=mpc.Kd, ground=default_plant())
    failed = torch.zeros(q.shape[0], dtype=torch.int32, device=d)
    period = float(mpc.config_gait.nominal_period)
    S = L.observe_rows(Q, V, replan * STEPS * mpc.sim_dt, mpc.sim_dt, period, collision_height=COLLISION_HEIGHT, failed=failed, step_index=replan)
    # the advance kernel: the solver bit (status NaN = 1, QP failure = 4), then the one stamping rule
    failed |= ((status == 1) | (status == 4)).to(torch.int32) * SOLVER
    stamp = ((failed & mask) != 0) & ((failed >> SHIFT) == 0)
    failed = torch.where(stamp, failed | ((replan + 1) << SHIFT), failed)
    # the observation of the final state
    L.observe(q, v, (replan + 1) * STEPS * mpc.sim_dt, period, torch.zeros(q.shape[0], 0, device=d), collision_height=COLLISION_HEIGHT,
              failed=failed, step_index=replan, term_mask=mask)
    return S, A, q, v, failed


# ---- one DAgger iteration on the plant ----------------------------------------------------------------------------------------------------
class Dagger:
    """B = 4 robots, 5 control steps of 20 substeps, an untrained policy, batches of 8: what `learning.dagger_iteration` is run on"""
    B, K, DT, N_SUB = 4, 5, 5e-4, 20
    T = K * N_SUB * DT
    SEED, BATCH = 7, 8

    @staticmethod
    def setup(dev, lying=None):
        from iterative_learning_nmpc_amd.database import DeviceDatabase
        from iterative_learning_nmpc_amd.torque import BatchedTorqueLayer
        from iterative_learning_nmpc_amd.workloads import quadruped_tree
        from tests.solve_helpers import policy_pair
        B = Dagger.B
        rng = np.random.default_rng(2)
        q0 = standing_start(B)[0]; q0[:, 6:] += rng.normal(0, 0.03, (B, 12))
        if lying is not None:
            q0[lying, 2] = 0.05                               # the trunk below the collision height of 0.08 m
        mpc = expert(dev, B, n_nodes=30)
        mpc.set_command(np.array([0.2, 0.0, 0.0]), 0.0)
        goal = np.tile(np.float32([0.2, 0.0, 0.0]), (B, 1))
        return dict(mpc=mpc, layer=BatchedTorqueLayer(**quadruped_tree(), device=dev), db=DeviceDatabase(limit=256, norm_input=False, device=dev),
                    policy=policy_pair(47, 12, 2, 64, False, 64, seed=3)[0], q0=q0, v0=np.zeros((B, 18)), goal=goal)


# ---- the scenarios every table per robot is put through -----------------------------------------------------------------------------------
# `name` is the table's name of `torque.TABLES`: `L.set_<name>` attaches `rows` and detaches with None, `L._<name>` is what is
# attached, and `<name>=rows` is the keyword of `learning.evaluate_policy`.  `w` is the module's World of B robots with q, v, tau,
# q_des, A and goal.  What differs in substance between tables (a register, a noise step, a `ground=` that is ignored) is not here.
def attached(L, name):
    return getattr(L, "_" + name)


def row_b_is_robot_bs(w, rows, spare, attach, name, integrator, perm, label):
    """step and track under the table `rows` through `attach(rows, robots)`, which also attaches whatever else the case has for
    those robots: row by row the call under the uniform table, finite, permuted by a permutation of robots and rows, unchanged by
    the `spare` rows behind, and not the call without the table"""
    import torch
    from tests.torque_helpers import same
    L, n = w.L, w.n
    dt = DT_IMPLICIT if integrator == "implicit" else DT
    run = lambda world=w: world.step(dt=dt) + world.track(dt=dt)      # noqa: E731
    try:
        L.set_integrator(integrator)
        everyone = np.arange(n)
        got, _ = held_row_by_row(run, lambda: attach(rows, everyone), lambda b: attach(np.tile(rows[b], (n, 1)), everyone), sorted({0, n // 2, n - 1}),
                                 NAMES + (TRACK_NAMES if w.record else TRACK_NAMES[:2]), label)
        assert all(bool(torch.isfinite(x).all()) for x in got)
        p = torch.as_tensor(perm, device=L.device)
        attach(rows[perm], perm)
        assert all(same(x[p], y) for x, y in zip(got, run(w.permuted(perm)))), (name, n, integrator, "permuted")
        attach(np.vstack([rows, spare]), everyone)
        assert all(same(x, y) for x, y in zip(got, run())), (name, n, integrator, "spare rows")
        if n > 1:                                         # and the rows matter
            getattr(L, "set_" + name)(None)
            assert not all(same(x, y) for x, y in zip(got, run()))
    finally:
        detach(L)


def attach_then_detach_gives_the_bits_from_before(w, name, rows, integrator):
    import torch
    from tests.torque_helpers import same
    L, policy = w.L, default_policy()
    L.set_integrator(integrator)
    calls = lambda: w.step() + w.track() + w.rollout(policy)      # noqa: E731
    before = calls()
    getattr(L, "set_" + name)(rows)
    assert attached(L, name) is not None
    during = calls()
    getattr(L, "set_" + name)(None)
    assert attached(L, name) is None
    after = calls()
    assert all(same(x, y) if x.is_floating_point() else torch.equal(x, y) for x, y in zip(before, after))
    assert not all(same(x, y) for x, y in zip(before[:5], during[:5]))


def policy_rollout_is_its_chain_of_public_calls(w, policy, name, rows, integrator=None):
    """the rollout under the table against observe -> forward -> contact_step, control step by control step, and a last flags-only
    observation; and not the rollout without the table"""
    import torch
    from tests.torque_helpers import same
    L, dt32 = w.L, float(np.float32(DT))
    if integrator is not None:
        L.set_integrator(integrator)
    getattr(L, "set_" + name)(rows)
    q, v = w.q, w.v
    failed = torch.zeros(w.n, dtype=torch.int32, device=L.device)
    S, A = [], []
    for k in range(ROLLOUT_STEPS):
        s, x = L.observe(q, v, T0 + (k * N_SUB) * dt32, PERIOD, w.goal, collision_height=HEIGHT, failed=failed, step_index=k, term_mask=MASK)
        a = policy.forward(x)
        q, v = L.contact_step(q, v, DT, N_SUB, tau_ff=w.tau, q_des=a, kp=KP, kd=KD)[:2]
        S.append(s); A.append(a)
    L.observe(q, v, T0 + (ROLLOUT_STEPS * N_SUB) * dt32, PERIOD, w.goal, collision_height=HEIGHT, failed=failed, step_index=ROLLOUT_STEPS, term_mask=MASK)
    got = w.rollout(policy)
    assert all(same(x, y) for x, y in zip(got[:4], (q, v, torch.stack(S, 1), torch.stack(A, 1)))) and torch.equal(got[4], failed)
    getattr(L, "set_" + name)(None)
    assert not same(w.rollout(policy)[0], got[0])                                      # the table matters


def nominal_model_does_not_read_the_table(w, dev, name, rows):
    """every call that describes the nominal tree or the nominal controller gives the same bits with the table attached, while a
    plant call does take it"""
    import torch
    from iterative_learning_nmpc_amd.torque import GroundContact
    from tests.torque_helpers import same
    L, B = w.L, w.n
    a = w.d(np.random.default_rng(3).uniform(-5, 5, (B, 18)).astype(np.float32))
    f = w.d(np.random.default_rng(4).uniform(-40, 80, (B, 4, 3)).astype(np.float32))
    tau = w.d(np.random.default_rng(5).uniform(-20, 20, (B, 12)).astype(np.float32))
    mpc = expert(dev, 2)
    q0, v0 = standing_start(2)
    o = plant_rollout(mpc, L, q0, v0, ONE)
    zoh = mpc.id_repeat[:STEPS]
    flat = lambda x: torch.cat([y.reshape(B, -1) for y in x], 1)      # noqa: E731

    def nominal():
        return dict(fd_step=flat(L.step(w.q, w.v, DT, 2, tau_ff=w.tau, q_des=w.q_des, kp=KP, kd=KD, f=f)),
                    fd_accel=L.forward_dynamics(w.q, w.v, tau, f), id_torques=L.id_torques(w.q, w.v, a, f),
                    mass_matrix=L.mass_matrix(w.q), centroidal=flat(L.centroidal(w.q, w.v, jacobian=True)),
                    state_momentum=L.state_momentum(w.q, w.v), contact_forces=L.contact_forces(w.q, w.v, GroundContact()),
                    pd_target_action=L.pd_target_action(tau, w.q, w.v, kp=KP, kd=KD),
                    plan_actions=L.plan_actions(o["X"], o["U"], zoh, mpc.config_opt.time_horizon / mpc.config_opt.n_nodes, mpc.sim_dt, kp=mpc.Kp, kd=mpc.Kd))

    without = nominal()
    bare = w.step()
    getattr(L, "set_" + name)(rows)
    under = nominal()
    assert not same(w.step()[0], bare[0])                 # the table is attached and a plant call takes it
    for call in without:
        assert same(without[call], under[call]), call
    assert list(without) == ["fd_step", "fd_accel", "id_torques", "mass_matrix", "centroidal", "state_momentum", "contact_forces", "pd_target_action",
                             "plan_actions"]


def evaluate_policy_attaches_and_detaches_the_table(w, policy, name, rows):
    """`evaluate_policy(<name>=rows)` is the rollout under the attached table and leaves nothing attached, also when the rollout
    raises; a table of the caller's is refused and stays"""
    import torch
    from iterative_learning_nmpc_amd.learning import evaluate_policy
    from tests.torque_helpers import same
    L, setter, T = w.L, getattr(w.L, "set_" + name), ROLLOUT_STEPS * N_SUB * DT
    before = w.step()
    setter(rows)
    q, v, S, A, failed = w.rollout(policy)
    setter(None)
    bare = w.rollout(policy)
    kw = dict(dt=DT, n_sub=N_SUB, tau_ff=w.tau, kp=KP, kd=KD, t0=T0, period=PERIOD, terminate_mask=MASK, collision_height=HEIGHT)
    out = evaluate_policy(L, policy, None, w.q, w.v, w.goal, T, **{name: rows}, **kw)
    assert same(out["S"], S) and same(out["A"], A) and same(out["q"], q) and same(out["v"], v) and torch.equal(out["failed"], failed)
    assert not same(out["q"], bare[0])
    assert attached(L, name) is None
    assert all(same(x, y) for x, y in zip(w.step(), before))                           # after the call the layer's step is the un-attached bits
    assert same(evaluate_policy(L, policy, None, w.q, w.v, w.goal, T, **kw)["q"], bare[0])      # nothing is attached
    # also when the rollout raises: a goal of the wrong batch is refused inside the try
    with pytest.raises(Exception):
        evaluate_policy(L, policy, None, w.q, w.v, w.goal[:5], T, **{name: rows}, **kw)
    assert attached(L, name) is None and same(w.rollout(policy)[0], bare[0])
    # a table of the caller's is not replaced
    setter(rows)
    mine = attached(L, name)
    with pytest.raises(ValueError, match="attached already"):
        evaluate_policy(L, policy, None, w.q, w.v, w.goal, T, **{name: rows}, **kw)
    assert attached(L, name) is mine and same(w.rollout(policy)[0], q)


def expert_on_the_plant_meets_the_table_of_its_layer(dev, L, name, rows):
    """B = 2, one replan: the plant-mode rollout with a table on its layer is the chain plan labels -> contact_track -> observe_rows
    under the same table (the check of tests/test_gpu_wb_plant_rollout.py), and not the rollout without; the labels of the first
    plan are the nominal expert's"""
    import torch
    from tests.torque_helpers import same
    q0, v0 = standing_start(2)
    try:
        bare = plant_rollout(expert(dev, 2), L, q0, v0, ONE)
        getattr(L, "set_" + name)(rows)
        mpc = expert(dev, 2)
        o = plant_rollout(mpc, L, q0, v0, ONE)
        S, A, q, v, failed = chain_of_public_calls(mpc, L, o["X"], o["U"], q0, v0, o["status"])
    finally:
        getattr(L, "set_" + name)(None)
    assert o["S"].shape == (2, STEPS, 44) and bool(torch.isfinite(o["S"]).all())
    assert all(same(a, b) for a, b in zip((o["S"], o["A"], o["q"], o["v"]), (S, A, q, v))) and torch.equal(o["failed"], failed)
    assert same(o["A"], bare["A"])                        # the labels of the first plan are the nominal expert's
    assert not same(o["q"], bare["q"])                    # the plant answered them under the table


def calls_beyond_the_tables_rows_are_refused(w, small, policy, name, table, *more):
    """with the device tensor `table` of small.n < w.n rows attached: every call of w that reads the table is refused under both
    integrators with its outputs untouched, n_rows < 1 and a NULL handle are refused through the raw library (`more`: what the
    setter of the library takes behind n_rows), and what is attached stays in force"""
    import torch
    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd._lib import NmpcError
    from tests.torque_helpers import same
    L, refusal, K = w.L, f"{name}: B exceeds n_rows", w.A.shape[1]
    raw = getattr(L.lib, "nmpc_contact_set_" + name)
    assert attached(L, name) is table                     # a device tensor is taken as given
    kept = small.step()
    for integrator in INTEGRATORS:
        L.set_integrator(integrator)
        for call in (w.step, w.track, lambda: w.rollout(policy)):
            with pytest.raises(NmpcError, match=refusal):
                call()
        q, v = w.q.clone(), w.v.clone()
        Q, V = torch.full((w.n, K, 18), 7.0, device=L.device), torch.full((w.n, K, 18), 7.0, device=L.device)
        with pytest.raises(NmpcError, match=refusal):
            L.contact_track(q, v, w.A, DT, N_SUB, tau_ff=w.tau, kp=KP, kd=KD, Q=Q, V=V)
        assert same(q, w.q) and same(v, w.v) and bool((Q == 7.0).all()) and bool((V == 7.0).all())
    L.set_integrator("explicit")
    assert all(same(x, y) for x, y in zip(small.step(), kept))
    for n_rows in (0, -3):
        assert raw(L._h, _lib.ptr(table), n_rows, *more) == -1 and "n_rows must be at least 1" in error_text(L)
    assert all(same(x, y) for x, y in zip(small.step(), kept))
    with pytest.raises(NmpcError, match=refusal):
        w.step()
    assert raw(None, _lib.ptr(table), small.n, *more) == -1 and b"handle" in L.lib.nmpc_torque_last_error(None)
    return kept
