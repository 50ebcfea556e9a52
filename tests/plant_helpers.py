"""What the contact-plant tests and the rollouts on the plant share (helper module, not collected by pytest): the plant's constants,
the host `Fixture` base, the device `World`, `detach` with its fixture, the row-by-row comparison of a call under a table per robot
with the same call under one row for all, and the set-up of the whole-body expert on the plant.  Draws, references, case tables and
assertions stay in the test files.

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
    L.set_payloads(None)
    L.set_grounds(None)
    L.set_push(None)                                      # with its windows
    L.set_rollout_states(None)
    L.set_integrator("explicit")


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
