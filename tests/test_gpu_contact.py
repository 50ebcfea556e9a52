"""GPU checks of the ground-contact plant of the torque layer (nmpc_foot_kinematics_batch, nmpc_contact_forces_batch,
nmpc_contact_step_batch) against tests/contact_reference.py (itself checked in tests/test_contact_reference.py).

The accuracy bar is the one of tests/test_gpu_fd.py: a device result is compared with the fp64 reference under
    max(1e-5 * scale, 4 x the deviation of the numpy-float32 run of the same reference loop from the fp64 run),
both computed here, never from the code under test; scale is the largest |reference| of the compared array.  Bit-for-bit
claims are array equality.  Every figure is printed before it is asserted."""
import copy
import ctypes
import os

import numpy as np
import pytest

from tests import contact_reference as cr
from tests import fd_reference as fr
from tests.plant_helpers import DT, KD, KP
from tests.torque_helpers import Case, bar, branches, general_tree_case, ground, held, host, layer

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contact_settle.npz")


class Cases(dict):
    def __missing__(self, key):
        self[key] = {"quadruped": lambda: Case(fr.quadruped(), 257, seed=257),
                     "tilted": lambda: Case(fr.quadruped(perturb=0.3), 257, seed=258),
                     "tree23": lambda: general_tree_case(fr.random_tree(), 96, seed=5),
                     "tree30": lambda: general_tree_case(fr.random_tree(n=30, seed=13, feet=(4, 29, 29, 17)), 40, seed=6)}[key]()
        return self[key]


@pytest.fixture(scope="module")
def cases():
    return Cases()


TREES = [("quadruped", 1), ("quadruped", 33), ("quadruped", 257), ("tilted", 1), ("tilted", 33), ("tilted", 257), ("tree23", 96), ("tree30", 40)]


# ---- 1. foot kinematics, 2. the law ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree,B", TREES)
def test_foot_kinematics_match_the_reference(cases, tree, B):
    """B = 1: a lone robot; 33: one past a block; 257: many blocks with a ragged tail; tree23: two feet on one body, a foot on
    joint 0, prismatic joints; tree30: the 16-robot block of the step, here the widest slice of the kinematics kernel."""
    c = cases[tree]
    pos, vel = host(*c.L.foot_kinematics(c.q[:B], c.v[:B]))
    assert pos.shape == vel.shape == (B, len(c.m.foot_joint), 3)
    print(f"{tree} B {B}")
    assert held("pos", pos, c.pos[:B], c.pos32[:B]) and held("vel", vel, c.vel[:B], c.vel32[:B])
    rest_pos, rest_vel = host(*c.L.foot_kinematics(c.q[:B]))
    assert np.array_equal(rest_pos, pos) and not np.any(rest_vel)


@pytest.mark.parametrize("tree,B", TREES)
def test_contact_forces_match_the_law_on_the_reference_kinematics(cases, tree, B):
    c = cases[tree]
    f, = host(c.L.contact_forces(c.q[:B], c.v[:B], ground(c.g)))
    off, pushed, leaving = branches(c.g, c.pos[:B], c.vel[:B], c.f[:B])
    print(f"{tree} B {B}: feet off the ground {off}, pushed {pushed}, leaving too fast to be pushed {leaving}")
    if B >= 33:
        assert off and pushed and leaving        # all three branches of the law (one robot alone cannot promise them)
    assert f.shape == (B, len(c.m.foot_joint), 3) and held("f", f, c.f[:B], c.f32[:B])
    assert np.all(f[..., 2] >= 0)


def test_no_force_above_the_ground_and_none_without_stiffness(cases):
    c, B = cases["tilted"], 33
    far = cr.Ground(ground_z=float(c.pos[:B, :, 2].min()) - 0.01)
    f, = host(c.L.contact_forces(c.q[:B], c.v[:B], ground(far)))
    assert np.array_equal(f, np.zeros_like(f))
    soft = cr.Ground(stiffness=0.0)
    f, = host(c.L.contact_forces(c.q[:B], c.v[:B], ground(soft)))
    assert np.array_equal(f, np.zeros_like(f))


# ---- 3. the step ----------------------------------------------------------------------------------------------------------------
class StepRun:
    """`n_sub` substeps of B robots through contact_step_ref in fp64 over fd_ref and in numpy float32 over aba."""
    def __init__(self, m, g, q, v, n_sub, tau_ff, q_des):
        self.kw = dict(tau_ff=tau_ff, q_des=q_des, kp=KP, kd=KD)
        self.q, self.v, self.n_sub, self.g = q, v, n_sub, g
        arg = lambda x, b: None if x is None else x[b]                                          # noqa: E731
        run = lambda **kw: [cr.contact_step_ref(m, g, q[b], v[b], DT, n_sub, arg(tau_ff, b), arg(q_des, b), KP, KD, **kw)  # noqa: E731
                            for b in range(len(q))]
        self.ref = [np.stack(x) for x in zip(*run())]
        self.f32 = [np.stack(x) for x in zip(*run(fd=fr.aba, dtype=np.float32))]

    def device(self, L, B=None, **kw):
        s = slice(0, B)
        args = {k: (None if x is None else x[s]) for k, x in self.kw.items() if k in ("tau_ff", "q_des")}
        return L.contact_step(self.q[s], self.v[s], DT, kw.get("n_sub", self.n_sub), kp=KP, kd=KD, ground=ground(self.g), **args)

    def holds(self, got, B=None):
        return all([held(name, x, r[:B], f[:B]) for name, x, r, f in zip(("q", "v", "a", "f", "tau"), got, self.ref, self.f32)])


def pd_inputs(c, B, seed):
    q_des = (c.q[:B, c.m.n - c.m.nu:] + np.random.default_rng(seed).uniform(-0.1, 0.1, (B, c.m.nu))).astype(np.float32)
    return c.q[:B], c.v[:B], c.tau[:B], q_des


@pytest.fixture(scope="module")
def one_substep(cases):
    c = cases["tilted"]
    q, v, tau, q_des = pd_inputs(c, 33, 1)
    return StepRun(c.m, c.g, q, v, 1, tau, q_des)


@pytest.mark.parametrize("B", [1, 33])
def test_one_substep_matches_the_reference(cases, one_substep, B):
    r = one_substep
    off, pushed, leaving = branches(r.g, cases["tilted"].pos[:33], cases["tilted"].vel[:33], r.ref[3])
    assert off and pushed and leaving
    got = host(*r.device(cases["tilted"].L, B))
    assert [x.shape for x in got] == [(B, 18)] * 3 + [(B, 4, 3), (B, 12)]
    print(f"one substep, B {B}")
    assert r.holds(got, B)


def test_one_substep_of_many_blocks_matches_the_reference(cases, one_substep):
    """B = 257: nine blocks, the last with one robot.  The reference is run for the first 33 rows (the fixture above) and for
    the last 33, which hold the last full block and the ragged tail; the rows between are the same code on other lanes."""
    c = cases["tilted"]
    q, v, tau, q_des = pd_inputs(c, 257, 1)
    tail = StepRun(c.m, c.g, q[224:], v[224:], 1, tau[224:], q_des[224:])
    off, pushed, leaving = branches(c.g, c.pos[224:], c.vel[224:], tail.ref[3])
    assert off and pushed and leaving
    got = host(*c.L.contact_step(q, v, DT, 1, tau_ff=tau, q_des=q_des, kp=KP, kd=KD, ground=ground(c.g)))
    assert [x.shape for x in got] == [(257, 18)] * 3 + [(257, 4, 3), (257, 12)]
    print("one substep, B 257: rows 0..32")
    head_ok = one_substep.holds([x[:33] for x in got])
    print("one substep, B 257: rows 224..256")
    assert head_ok and tail.holds([x[224:] for x in got])


# the general trees under the step: the recursion carries the world position of the bodies itself (two feet on one body, a foot
# on joint 0, prismatic joints inside the tree), and the 30-joint tree runs the 16-robot block.  Their feet lie up to a metre
# in the ground, so the ground is soft enough for the explicit step (k delta c dt / m_foot < 2 with bodies of 0.1 kg).
SOFT = dict(stiffness=200.0, damping=0.5)
GENERAL = {"tree23": (33, 8), "tree30": (40, 17)}      # robots of the one-substep run and of the three-substep run


@pytest.fixture(scope="module")
def general_steps(cases):
    class Runs(dict):
        """tree -> (ground, the one-substep run, the three-substep run), built when first asked for"""
        def __missing__(self, tree):
            c, (B1, B3) = cases[tree], GENERAL[tree]
            g = cr.Ground(ground_z=c.g.ground_z, **SOFT)
            q, v, tau, q_des = pd_inputs(c, B1, 3)
            self[tree] = (g, StepRun(c.m, g, q, v, 1, tau, q_des), StepRun(c.m, g, q[:B3], v[:B3], 3, tau[:B3], q_des[:B3]))
            return self[tree]
    return Runs()


@pytest.mark.parametrize("tree", list(GENERAL))
def test_general_trees_step_as_the_reference(cases, general_steps, tree):
    """tree23: B = 33, one past a 32-robot block.  tree30: the 16-robot block; B = 40 is two and a half of them, B = 17 one and
    a robot."""
    c, (g, one, three) = cases[tree], general_steps[tree]
    B1, B3 = GENERAL[tree]
    n, nf = c.m.n, len(c.m.foot_joint)
    off, pushed, leaving = branches(g, c.pos[:B1], c.vel[:B1], one.ref[3])
    print(f"{tree}: feet off the ground {off}, pushed {pushed}, leaving too fast to be pushed {leaving}")
    assert off and pushed and leaving
    got = host(*one.device(c.L))
    assert [x.shape for x in got] == [(B1, n)] * 3 + [(B1, nf, 3), (B1, n)]
    print(f"{tree}: one substep, B {B1}")
    ok = one.holds(got)
    print(f"{tree}: three substeps, B {B3}")
    assert three.holds(host(*three.device(c.L))) and ok
    # the law in the step is the law of the forces call, on the same state
    f, = host(c.L.contact_forces(one.q, one.v, ground(g)))
    assert held("f of the step against contact_forces", got[3], f.astype(np.float64), f)


def test_a_row_does_not_depend_on_its_batch(cases, one_substep):
    """257 robots: nine blocks, the last with one robot; its rows are those of the 33-robot call and of calls of one."""
    c, r = cases["tilted"], one_substep
    q, v, tau, q_des = pd_inputs(c, 257, 1)
    kw = dict(kp=KP, kd=KD, ground=ground(c.g))
    whole = host(*c.L.contact_step(q, v, DT, 3, tau_ff=tau, q_des=q_des, **kw))
    part = host(*c.L.contact_step(q[:33], v[:33], DT, 3, tau_ff=tau[:33], q_des=q_des[:33], **kw))
    assert all(np.array_equal(x[:33], y) for x, y in zip(whole, part))
    for b in (0, 31, 32, 255, 256):
        row = host(*c.L.contact_step(q[b:b + 1], v[b:b + 1], DT, 3, tau_ff=tau[b:b + 1], q_des=q_des[b:b + 1], **kw))
        assert all(np.array_equal(x[0], y[b]) for x, y in zip(row, whole)), b
    assert np.array_equal(host(*r.device(c.L))[0], host(*c.L.contact_step(q[:33], v[:33], DT, 1, tau_ff=tau[:33], q_des=q_des[:33], **kw))[0])


@pytest.fixture(scope="module")
def touch_down():
    """Three quadrupeds around the standing pose, the lowest foot 5 mm above the ground, sinking at 0.5 m/s: forty substeps
    of 0.5 ms cross touch-down after about ten milliseconds."""
    d, B, rng = cr.drop(), 3, np.random.default_rng(40)
    m = d["m"]
    q = np.tile(d["q"].astype(np.float64), (B, 1))
    q[:, 6:] += rng.uniform(-0.1, 0.1, (B, 12))
    for b in range(B):
        q[b, 2] += 0.005 - cr.feet(m, q[b])[0][:, 2].min()
    v = rng.uniform(-0.2, 0.2, (B, 18)); v[:, 2] = -0.5
    q, v = q.astype(np.float32), v.astype(np.float32)
    return StepRun(m, d["g"], q, v, 40, np.tile(d["tau_ff"], (B, 1)), np.tile(d["q_des"], (B, 1)))


def test_forty_substeps_across_touch_down(cases, touch_down):
    r, m = touch_down, cases["quadruped"].m
    start = np.stack([cr.contact_law(r.g, *cr.feet(m, r.q[b], r.v[b])) for b in range(len(r.q))])
    assert not np.any(start) and np.all(r.ref[3][..., 2].max(axis=1) > 0)          # the run starts in the air and ends on the ground
    print("forty substeps across touch-down")
    assert r.holds(host(*r.device(cases["quadruped"].L)))


def test_twenty_substeps_are_twenty_calls_of_one(cases, touch_down):
    r, L = touch_down, cases["quadruped"].L
    q0, v0 = r.q.copy(), r.v.copy(); v0[:, 2] = -2.0                               # on the ground within the twenty
    kw = dict(tau_ff=r.kw["tau_ff"], q_des=r.kw["q_des"], kp=KP, kd=KD, ground=ground(r.g))
    once = L.contact_step(q0, v0, DT, 20, **kw)
    q, v, out = q0, v0, None
    for _ in range(20):
        out = L.contact_step(q, v, DT, 1, **kw)
        q, v = out[0], out[1]
    assert bool((once[3][..., 2] > 0).any())
    assert all(torch.equal(x, y) for x, y in zip(out, once))


def test_outputs_may_alias_the_inputs(cases, one_substep):
    from iterative_learning_nmpc_amd import _lib
    r, L = one_substep, cases["tilted"].L
    apart = r.device(L, n_sub=5)
    q, v, tau, q_des = (torch.as_tensor(x, device=L.device).contiguous() for x in (r.q, r.v, r.kw["tau_ff"], r.kw["q_des"]))
    B = q.shape[0]
    a, f, t = torch.empty_like(q), torch.empty(B, 4, 3, device=L.device), torch.empty(B, 12, device=L.device)
    ptr, cfg = _lib.ptr, ground(r.g).cfg()
    _lib.check(L.lib.nmpc_contact_step_batch(L._h, B, 5, DT, ctypes.byref(cfg), ptr(q), ptr(v), ptr(tau), ptr(q_des), KP, KD, ptr(q), ptr(v),
                                             ptr(a), ptr(f), ptr(t), _lib.stream(L.device)), L._h, "nmpc_contact_step_batch", "torque")
    assert all(torch.equal(x, y) for x, y in zip((q, v, a, f, t), apart))
    # the optional outputs left out: the state is the same
    q2, v2 = (torch.as_tensor(x, device=L.device).contiguous() for x in (r.q, r.v))
    _lib.check(L.lib.nmpc_contact_step_batch(L._h, B, 5, DT, ctypes.byref(cfg), ptr(q2), ptr(v2), ptr(tau), ptr(q_des), KP, KD, ptr(q2), ptr(v2),
                                             None, None, None, _lib.stream(L.device)), L._h, "nmpc_contact_step_batch", "torque")
    assert torch.equal(q2, q) and torch.equal(v2, v)


def test_far_above_the_ground_the_step_is_the_step_without_forces(cases):
    """Another kernel than nmpc_fd_step_batch, so its bits are not asked for: the reference of `step` with f = 0 is."""
    c, B, K = cases["tilted"], 8, 4
    q, v, tau, q_des = pd_inputs(c, B, 2)
    zero = np.zeros((4, 3))
    ref = [np.stack(x) for x in zip(*[fr.step_ref(c.m, q[b], v[b], DT, K, tau[b], q_des[b], KP, KD, zero) for b in range(B)])]
    f32 = [np.stack(x) for x in zip(*[fr.step_ref(c.m, q[b], v[b], DT, K, tau[b], q_des[b], KP, KD, zero, fd=fr.aba, dtype=np.float32)
                                      for b in range(B)])]
    got = host(*c.L.contact_step(q, v, DT, K, tau_ff=tau, q_des=q_des, kp=KP, kd=KD, ground=ground(cr.Ground(ground_z=-10.0))))
    print("far above the ground")
    assert all([held(name, x, r, f) for name, x, r, f in zip(("q", "v", "a"), got, ref, f32)])
    assert np.array_equal(got[3], np.zeros((B, 4, 3), np.float32))


def test_the_torque_limit(cases, one_substep):
    c, free = cases["tilted"], one_substep
    g = cr.Ground(tau_max=5.0)
    r = StepRun(c.m, g, free.q, free.v, 1, free.kw["tau_ff"], free.kw["q_des"])
    got = host(*r.device(c.L))
    tau, unclamped = got[4], host(*free.device(c.L))[4]
    inside = np.abs(unclamped) < 5.0
    print(f"torque limit: {int((~inside).sum())} of {inside.size} torques clamped")
    assert inside.any() and (~inside).any()
    assert np.all(np.abs(tau) <= 5.0) and np.array_equal(tau[inside], unclamped[inside])
    assert np.array_equal(tau[~inside], np.float32(5.0) * np.sign(unclamped[~inside]))
    assert r.holds(got)
    # a torque that is not a number stays none: the limit does not turn bad input into a saturated torque
    bad = free.kw["tau_ff"].copy(); bad[0, 3] = np.nan
    spoilt = host(*c.L.contact_step(free.q, free.v, DT, 1, tau_ff=bad, q_des=free.kw["q_des"], kp=KP, kd=KD, ground=ground(g)))
    assert np.isnan(spoilt[4][0, 3]) and np.isnan(spoilt[2][0]).any()
    assert all(np.array_equal(x[1:], y[1:]) for x, y in zip(spoilt, got))


# ---- 4. settling ----------------------------------------------------------------------------------------------------------------
def test_the_dropped_quadruped_settles_as_the_reference(cases):
    """tests/golden/contact_settle.npz: 2 000 substeps of 0.5 ms in one call, two identical rows."""
    s, L = np.load(GOLDEN), cases["quadruped"].L
    two = lambda x: np.tile(x, (2, 1))                                             # noqa: E731
    q, v, a, f, tau = host(*L.contact_step(two(s["q0"]), two(s["v0"]), float(s["dt"]), int(s["n_sub"]), tau_ff=two(s["tau_ff"]),
                                           q_des=two(s["q_des"]), kp=float(s["kp"]), kd=float(s["kd"])))
    assert all(np.array_equal(x[0], x[1]) for x in (q, v, a, f, tau))
    print("settling, 2 000 substeps")
    ok = [held(k, x[0], s[k], s[k + "32"]) for k, x in (("q", q), ("v", v), ("f", f))]
    weight = cases["quadruped"].m.mass.sum() * fr.G
    print(f"  sum f_z {f[0, :, 2].sum():.4f} N, weight {weight:.4f} N, reference {s['f'][:, 2].sum():.4f} N")
    assert all(ok)
    assert abs(f[0, :, 2].sum() - weight) < 1e-3 * weight + bar(s["f"], s["f32"])
    assert np.all(f[0, :, 2] > 0) and np.abs(v).max() < 1e-2 + bar(s["v"], s["v32"])


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------
def test_errors_and_the_empty_batch(cases):
    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd._lib import NmpcError
    from iterative_learning_nmpc_amd.torque import GroundContact
    c = cases["quadruped"]
    L, q, v = c.L, c.q[:2], c.v[:2]
    with pytest.raises(NmpcError, match="n_sub must be at least 1"):
        L.contact_step(q, v, DT, 0)
    with pytest.raises(NmpcError, match="dt must be positive"):
        L.contact_step(q, v, 0.0)
    refused = [(dict(stiffness=-1.0), "must not be negative"), (dict(damping=-0.1), "must not be negative"), (dict(mu=-0.5), "must not be negative"),
               (dict(slip_velocity=0.0), "slip_velocity must be positive"), (dict(slip_velocity=-1.0), "slip_velocity must be positive"),
               (dict(ground_z=float("nan")), "must be finite"), (dict(stiffness=float("inf")), "must be finite"),
               (dict(tau_max=float("nan")), "must be finite"), (dict(slip_velocity=float("inf")), "must be finite")]
    for fields, text in refused:
        with pytest.raises(NmpcError, match=text):
            L.contact_step(q, v, DT, ground=GroundContact(**fields))
        with pytest.raises(NmpcError, match=text):
            L.contact_forces(q, v, GroundContact(**fields))
    # NULL arguments, at the C boundary
    t = lambda x: torch.as_tensor(x, device=L.device).contiguous()                 # noqa: E731
    qd, vd, out, f = t(q), t(v), torch.empty(2, 18, device=L.device), torch.empty(2, 4, 3, device=L.device)
    ptr, cfg, st = _lib.ptr, ctypes.byref(GroundContact().cfg()), _lib.stream(L.device)
    step = lambda cfg, q, v, qo, vo: L.lib.nmpc_contact_step_batch(L._h, 2, 1, DT, cfg, q, v, None, None, KP, KD, qo, vo, None, None, None, st)  # noqa: E731
    for args, text in (((None, ptr(qd), ptr(vd), ptr(out), ptr(out)), "cfg is NULL"), ((cfg, None, ptr(vd), ptr(out), ptr(out)), "need B >= 0 and q, v"),
                       ((cfg, ptr(qd), None, ptr(out), ptr(out)), "need B >= 0 and q, v"), ((cfg, ptr(qd), ptr(vd), None, ptr(out)), "q_out"),
                       ((cfg, ptr(qd), ptr(vd), ptr(out), None), "v_out")):
        assert step(*args) == -1 and text in L.lib.nmpc_torque_last_error(L._h).decode()
    assert L.lib.nmpc_contact_forces_batch(L._h, 2, None, ptr(qd), ptr(vd), ptr(f), st) == -1 and "cfg is NULL" in L.lib.nmpc_torque_last_error(L._h).decode()
    assert L.lib.nmpc_contact_forces_batch(L._h, 2, cfg, None, ptr(vd), ptr(f), st) == -1
    assert L.lib.nmpc_contact_forces_batch(L._h, 2, cfg, ptr(qd), ptr(vd), None, st) == -1 and "q, f" in L.lib.nmpc_torque_last_error(L._h).decode()
    assert L.lib.nmpc_foot_kinematics_batch(L._h, 2, None, None, ptr(f), ptr(f), st) == -1
    assert L.lib.nmpc_foot_kinematics_batch(L._h, 2, ptr(qd), None, None, None, st) == -1 and "pos or vel" in L.lib.nmpc_torque_last_error(L._h).decode()
    # one of pos, vel is enough
    only = torch.empty(2, 4, 3, device=L.device)
    assert L.lib.nmpc_foot_kinematics_batch(L._h, 2, ptr(qd), ptr(vd), None, ptr(only), st) == 0
    assert torch.equal(only, L.foot_kinematics(q, v)[1])
    # the layer's own checks
    with pytest.raises(ValueError, match="expected"):
        L.foot_kinematics(q[:, :17])
    with pytest.raises(ValueError, match="expected"):
        L.contact_step(q, v, DT, q_des=np.zeros((2, 18), np.float32))
    with pytest.raises(ValueError, match="batch sizes"):
        L.contact_forces(q, c.v[:3], GroundContact())
    # B = 0
    assert [tuple(x.shape) for x in L.foot_kinematics(q[:0], v[:0])] == [(0, 4, 3)] * 2
    assert L.contact_forces(q[:0], v[:0], GroundContact()).shape == (0, 4, 3)
    assert [tuple(x.shape) for x in L.contact_step(q[:0], v[:0], DT, 3)] == [(0, 18)] * 3 + [(0, 4, 3), (0, 12)]


def test_massless_leaf_gives_nan_rows_and_the_next_call_is_sound(cases, one_substep):
    c, B = cases["quadruped"], 33
    bad = copy.deepcopy(c.m)
    bad.mass[17] = 0.0; bad.inertia[17] = 0.0
    out = host(*layer(bad).contact_step(c.q[:B], c.v[:B], DT, 2, tau_ff=c.tau[:B]))
    assert [x.shape for x in out] == [(B, 18)] * 3 + [(B, 4, 3), (B, 12)] and all(np.isnan(x).all() for x in out)
    print("after the NaN rows")
    assert one_substep.holds(host(*one_substep.device(cases["tilted"].L)))
